"""Inputs for the direct gzip / snappy page-decoder tests.

Everything here is host-only and deterministic. tests/test_codec_cases_cpu.py
checks every stream against zlib / pyarrow and the RFC walker without a
GPU; tests/test_gpu_codecs.py feeds the same streams to qk_gzip_pages and
qk_snappy_pages. Building them in one place guarantees both see the same
bytes.
"""
import functools
import struct
import zlib

import numpy as np

TEXT = b"the quick brown fox 64 " * 64          # 1472 bytes


# ---- payload families ---------------------------------------------------

@functools.lru_cache(maxsize=None)
def payloads():
    rng = np.random.default_rng(20240611)

    def rand(n):
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    two = bytearray()
    while len(two) < 2000:
        two += bytes([0x41 + (len(two) & 1)]) * int(rng.integers(1, 40))
    # geometric histogram over all 256 byte values: the rarest symbols
    # occur once among ~7600, so a Huffman code built from it needs codes
    # well past 10 bits
    counts = np.maximum(1, np.round(300 * 0.96 ** np.arange(256)))
    skew = np.repeat(np.arange(256, dtype=np.uint8), counts.astype(int))
    rng.shuffle(skew)
    block = rand(300)
    return {
        "const": b"\x5a" * 2500,
        "two": bytes(two[:2000]),
        "text": TEXT,
        "random": rand(1800),
        "rand_text": rand(900) + TEXT[:1150],
        "text_rand": TEXT[:1150] + rand(900),
        "skew": skew.tobytes(),
        "dist32k": block + rand(32768 - 300) + block,
        "empty": b"",
    }


LEVELS = (0, 1, 6, 9)
STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "fixed": zlib.Z_FIXED,
              "rle": zlib.Z_RLE, "huff": zlib.Z_HUFFMAN_ONLY}
FLUSHES = {"full": zlib.Z_FULL_FLUSH, "sync": zlib.Z_SYNC_FLUSH}


def deflate(payload, level, strategy, flush=None, at=None):
    """Raw deflate of payload; optionally flush(kind) after `at` bytes."""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    if flush is None:
        return c.compress(payload) + c.flush()
    return (c.compress(payload[:at]) + c.flush(flush)
            + c.compress(payload[at:]) + c.flush())


class GzCase:
    __slots__ = ("name", "payload", "raw")

    def __init__(self, name, payload, raw):
        self.name, self.payload, self.raw = name, payload, raw

    def __repr__(self):
        return "GzCase(%s)" % self.name


EXAMPLE = "text-L6-rle-full@1471"     # the stream quoted in the docstring
#   of test_gpu_codecs.test_gzip_flushed_example: Huffman block, then the
#   empty stored block of a full flush before the last payload byte


@functools.lru_cache(maxsize=None)
def gzip_matrix():
    """levels x strategies x (no flush | full/sync flush at byte 1, the
    middle, len-1 and len) over the small payload families."""
    P = payloads()
    cases = []
    for fam in ("const", "two", "text", "random", "rand_text", "text_rand",
                "skew"):
        p = P[fam]
        n = len(p)
        for level in LEVELS:
            for sname, strat in STRATEGIES.items():
                tag = "%s-L%d-%s" % (fam, level, sname)
                cases.append(GzCase(tag, p, deflate(p, level, strat)))
                for fname, fl in FLUSHES.items():
                    for at in (1, n // 2, n - 1, n):
                        cases.append(GzCase(
                            "%s-%s@%d" % (tag, fname, at), p,
                            deflate(p, level, strat, fl, at)))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def walks():
    """name -> RFC walker result for every matrix and special stream
    (walked once per process; the pure-Python walk is the slow part)."""
    from _deflate_walker import walk
    out = {c.name: walk(c.raw) for c in gzip_matrix()}
    out.update((c.name, walk(c.raw)) for c in gzip_special().values())
    return out


def fixed_block_cases():
    """Matrix streams that must contain a fixed-Huffman block:
    compressible payloads under Z_FIXED at a level that compresses."""
    return [c for c in gzip_matrix()
            if c.name.split("-")[0] in ("const", "two", "text")
            and "-fixed" in c.name and "-L0-" not in c.name]


def long_code_cases():
    """Matrix streams that must use literal codes longer than 10 bits:
    the skewed histogram, Huffman only."""
    return [c for c in gzip_matrix()
            if c.name.startswith("skew-") and "-huff" in c.name
            and "-L0-" not in c.name]


# ---- hand-emitted fixed-Huffman stream ----------------------------------
# zlib never emits distance 32768 (its window keeps a 262-byte lookahead
# margin), so the one stream that needs it is written bit by bit here,
# straight from RFC 1951 3.2.6.

class _BitWriter:
    def __init__(self):
        self.acc = 0
        self.n = 0

    def bits(self, value, nbits):          # data field, LSB first
        self.acc |= value << self.n
        self.n += nbits

    def code(self, value, nbits):          # Huffman code, MSB first
        for i in range(nbits - 1, -1, -1):
            self.bits((value >> i) & 1, 1)

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def _fixed_lit(w, sym):
    if sym < 144:
        w.code(0x30 + sym, 8)
    elif sym < 256:
        w.code(0x190 + sym - 144, 9)
    elif sym < 280:
        w.code(sym - 256, 7)
    else:
        w.code(0xC0 + sym - 280, 8)


def fixed_stream(ops):
    """One final fixed-Huffman block. ops: bytes objects (literals) or
    (length, distance) pairs; only lengths 3..10 and 258 and distances
    1..4 and 32768 are needed, so only those are encoded."""
    w = _BitWriter()
    w.bits(1, 1)
    w.bits(1, 2)
    for op in ops:
        if isinstance(op, bytes):
            for b in op:
                _fixed_lit(w, b)
            continue
        length, dist = op
        if 3 <= length <= 10:
            _fixed_lit(w, 254 + length)
        elif length == 258:
            _fixed_lit(w, 285)
        else:
            raise ValueError(length)
        if 1 <= dist <= 4:
            w.code(dist - 1, 5)
        elif dist == 32768:
            w.code(29, 5)                  # base 24577, 13 extra bits
            w.bits(32768 - 24577, 13)
        else:
            raise ValueError(dist)
    _fixed_lit(w, 256)
    return w.bytes()


def _apply(ops):
    out = bytearray()
    for op in ops:
        if isinstance(op, bytes):
            out += op
        else:
            for _ in range(op[0]):
                out.append(out[-op[1]])
    return bytes(out)


@functools.lru_cache(maxsize=None)
def gzip_special():
    """Streams outside the matrix, each named for the path it reaches."""
    P = payloads()
    rng = np.random.default_rng(7)
    out = {}
    out["empty"] = GzCase("empty", b"", deflate(b"", 6, 0))
    for n in (65535, 65536, 70000):
        p = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        out["stored%d" % n] = GzCase("stored%d" % n, p, deflate(p, 0, 0))
    for level in (1, 6, 9):
        out["dist32k-L%d" % level] = GzCase(
            "dist32k-L%d" % level, P["dist32k"],
            deflate(P["dist32k"], level, 0))
    ops = (P["dist32k"][:32768], (258, 32768), (10, 32768), b"xyz",
           (3, 1), (258, 4))
    out["fixed-maxdist"] = GzCase("fixed-maxdist", _apply(ops),
                                  fixed_stream(ops))
    # run of one byte: zlib's longest match, length 258 at distance 1
    p = b"\x00" * 5000
    out["maxlen"] = GzCase("maxlen", p, deflate(p, 9, 0))
    # natural (unflushed) Huffman-then-stored: compressible text, then
    # enough random bytes that zlib stores the second block
    p = TEXT * 12 + rng.integers(0, 256, 40000, dtype=np.uint8).tobytes()
    out["natural-huff-stored"] = GzCase("natural-huff-stored", p,
                                        deflate(p, 6, 0))
    return out


# ---- gzip wrapper (RFC 1952) --------------------------------------------

FEXTRA, FNAME, FCOMMENT, FHCRC = 4, 8, 16, 2
ALL_FLAGS = tuple(a | b | c | d for a in (0, FEXTRA) for b in (0, FNAME)
                  for c in (0, FCOMMENT) for d in (0, FHCRC))


def gzip_wrap(raw, payload, flags=0):
    """10-byte header + optional fields + raw deflate + CRC32/ISIZE."""
    h = bytearray([0x1F, 0x8B, 8, flags, 0x78, 0x56, 0x34, 0x12, 0, 3])
    if flags & FEXTRA:
        extra = b"QK\x05\x00\x00\x01\x02\x03\x04"   # holds zero bytes
        h += struct.pack("<H", len(extra)) + extra
    if flags & FNAME:
        h += b"page.bin\x00"
    if flags & FCOMMENT:
        h += b"a comment\x00"
    if flags & FHCRC:
        h += struct.pack("<H", zlib.crc32(bytes(h)) & 0xFFFF)
    return bytes(h) + raw + struct.pack("<II", zlib.crc32(payload),
                                        len(payload) & 0xFFFFFFFF)


# ---- snappy element emitter ---------------------------------------------

def varint(n):
    out = bytearray()
    while n >= 0x80:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


class Snappy:
    """Writes snappy elements one by one and keeps the bytes they decode
    to. `form` forces a literal's length field to 0 (in the tag) or 1..4
    extra bytes; the format allows a wider field than needed."""

    def __init__(self):
        self.el = bytearray()
        self.out = bytearray()
        self.kinds = []

    def literal(self, data, form=None):
        n = len(data) - 1
        need = 0 if n < 60 else (n.bit_length() + 7) // 8
        form = need if form is None else form
        assert form >= need and n >= 0
        if form == 0:
            self.el.append(n << 2)
        else:
            self.el.append((59 + form) << 2)
            self.el += n.to_bytes(form, "little")
        self.el += data
        self.out += data
        self.kinds.append("lit%d" % form)
        return self

    def _copy(self, off, ln):
        assert 0 < off <= len(self.out)
        for _ in range(ln):
            self.out.append(self.out[-off])

    def copy1(self, off, ln):
        assert 4 <= ln <= 11 and off < 2048
        self.el += bytes([1 | ((ln - 4) << 2) | ((off >> 8) << 5),
                          off & 0xFF])
        self._copy(off, ln)
        self.kinds.append("copy1")
        return self

    def copy2(self, off, ln):
        assert 1 <= ln <= 64 and off < 65536
        self.el += bytes([2 | ((ln - 1) << 2)]) + struct.pack("<H", off)
        self._copy(off, ln)
        self.kinds.append("copy2")
        return self

    def copy4(self, off, ln):
        assert 1 <= ln <= 64
        self.el += bytes([3 | ((ln - 1) << 2)]) + struct.pack("<I", off)
        self._copy(off, ln)
        self.kinds.append("copy4")
        return self

    def stream(self):
        return varint(len(self.out)) + bytes(self.el)

    def expected(self):
        return bytes(self.out)


class SnCase:
    __slots__ = ("name", "stream", "expected", "kinds")

    def __init__(self, name, s):
        self.name = name
        self.stream = s.stream()
        self.expected = s.expected()
        self.kinds = tuple(s.kinds)

    def __repr__(self):
        return "SnCase(%s)" % self.name


LITERAL_LENGTHS = (1, 59, 60, 61, 255, 256, 257, 65535, 65536, 65537)
OVERLAP_OFFSETS = (1, 2, 3, 7, 63, 64, 65)


@functools.lru_cache(maxsize=None)
def snappy_valid():
    rng = np.random.default_rng(99)

    def rand(n):
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    cases = []

    def add(name, s):
        cases.append(SnCase(name, s))

    for n in LITERAL_LENGTHS:
        add("lit%d" % n, Snappy().literal(rand(n)))
    # wider length fields than needed, up to the 4-byte form
    add("lit61-form2", Snappy().literal(rand(61), form=2))
    add("lit257-form3", Snappy().literal(rand(257), form=3))
    add("lit65537-form4", Snappy().literal(rand(65537), form=4))
    add("lit1-form4", Snappy().literal(b"\x42", form=4))
    base = rand(2100)
    for ln in range(4, 12):
        for off in (1, 2, 255, 256, 2047):
            add("copy1-len%d-off%d" % (ln, off),
                Snappy().literal(base).copy1(off, ln))
    big = rand(65600)
    for ln in (1, 64):
        for off in (1, 2048, 65535):
            add("copy2-len%d-off%d" % (ln, off),
                Snappy().literal(big[:max(off, 8)]).copy2(off, ln))
    s = Snappy().literal(rand(70000))
    s.copy4(65536, 64).copy4(69999, 37).literal(rand(5)).copy4(70000, 1)
    s.copy4(65536, 11)
    add("copy4-70k", s)
    seed = rand(70)
    for ln in (64, 11, 5):
        for off in OVERLAP_OFFSETS:
            add("overlap-copy2-len%d-off%d" % (ln, off),
                Snappy().literal(seed).copy2(off, ln).literal(b"\xEE"))
            if ln <= 11:
                add("overlap-copy1-len%d-off%d" % (ln, off),
                    Snappy().literal(seed).copy1(off, ln))
    # a copy that reads the literal just before it, a literal right after
    # a copy, and a copy that reads the previous copy's output
    s = Snappy().literal(rand(10)).copy1(5, 8).literal(rand(7))
    s.copy2(3, 20).copy2(20, 20).literal(rand(3)).copy1(1, 11)
    add("interleaved", s)
    return tuple(cases)


# ---- v1 definition levels, max level 1 (parquet Encodings.md, RLE) ------

def bit_packed(bits):
    """One bit-packed run of width 1; len(bits) is a multiple of 8."""
    assert len(bits) % 8 == 0
    body = bytearray()
    for g in range(0, len(bits), 8):
        body.append(sum(b << i for i, b in enumerate(bits[g:g + 8])))
    return varint(((len(bits) // 8) << 1) | 1) + bytes(body)


def fill_run(count, value):
    return varint(count << 1) + bytes([value])


def levels_page(runs, values, claimed_len=None):
    """v1 data page body: [u32 len][RLE/bit-packed runs][values]."""
    ln = len(runs) if claimed_len is None else claimed_len
    return struct.pack("<I", ln) + runs + values


class LvCase:
    """page: decompressed page bytes; err / data_off / first: what both
    the kernel and the host mirror must report for it."""
    __slots__ = ("name", "page", "num_values", "err", "data_off", "first")

    def __init__(self, name, runs, num_values, err, values=b"\x07values",
                 claimed_len=None):
        self.name = name
        self.page = levels_page(runs, values, claimed_len)
        self.num_values = num_values
        self.err = err
        self.data_off = 4 + (len(runs) if claimed_len is None
                             else claimed_len)
        ok = err == 0 and self.data_off < len(self.page)
        self.first = self.page[self.data_off] if ok else -1

    def __repr__(self):
        return "LvCase(%s)" % self.name


def _ones(n, zero_at=(), pad=1):
    """n valid levels of 1 (0 at the given positions), padded to whole
    groups of 8 with `pad`."""
    bits = [1] * n + [pad] * (-n % 8)
    for z in zero_at:
        bits[z] = 0
    return bits


@functools.lru_cache(maxsize=None)
def levels_cases():
    bp = bit_packed
    mixed = bp(_ones(16)) + fill_run(30, 1) + bp(_ones(5))
    return (
        LvCase("bp-64", bp(_ones(64)), 64, 0),
        LvCase("bp-61", bp(_ones(61)), 61, 0),
        LvCase("bp-5", bp(_ones(5)), 5, 0),
        LvCase("bp-520-header2", bp(_ones(520)), 520, 0),
        LvCase("bp-517-header2", bp(_ones(517)), 517, 0),
        LvCase("fill-7", fill_run(7, 1), 7, 0),
        LvCase("fill-100-header2", fill_run(100, 1), 100, 0),
        LvCase("fill-20000-header3", fill_run(20000, 1), 20000, 0),
        LvCase("mixed", mixed, 51, 0),
        LvCase("mixed-fill-first",
               fill_run(3, 1) + bp(_ones(64)) + fill_run(200, 1), 267, 0),
        LvCase("no-values-after-levels", bp(_ones(8)), 8, 0, values=b""),
        LvCase("run-past-num-values-ignored",
               bp(_ones(64)) + fill_run(5, 0), 64, 0),
        LvCase("fill0-count0", fill_run(0, 0) + fill_run(8, 1), 8, 0),
        # 0 bits only in the padding beyond num_values: accepted
        LvCase("pad-zero-61", bp(_ones(61, pad=0)), 61, 0),
        LvCase("pad-zero-5", bp(_ones(5, pad=0)), 5, 0),
        LvCase("pad-zero-mixed",
               bp(_ones(16)) + fill_run(30, 1) + bp(_ones(5, pad=0)), 51, 0),
        # a single null
        LvCase("null-first", bp(_ones(61, zero_at=(0,))), 61, 3),
        LvCase("null-middle", bp(_ones(61, zero_at=(30,))), 61, 3),
        LvCase("null-last-valid", bp(_ones(61, zero_at=(60,))), 61, 3),
        LvCase("null-last-64", bp(_ones(64, zero_at=(63,))), 64, 3),
        LvCase("null-mixed-last",
               bp(_ones(16)) + fill_run(30, 1) + bp(_ones(5, zero_at=(4,))),
               51, 3),
        LvCase("null-fill", fill_run(9, 0), 9, 3),
        LvCase("null-fill-after-bp", bp(_ones(8)) + fill_run(4, 0), 12, 3),
        # levels length pointing past the page
        LvCase("len-past-page", bp(_ones(8)), 8, 1, claimed_len=60),
    )


def literal_only(data):
    """Snappy stream holding `data` as literals of at most 60 bytes."""
    s = Snappy()
    for i in range(0, len(data), 60):
        s.literal(data[i:i + 60])
    return s.stream()


# ---- streams the decoders must refuse -----------------------------------

class Refused:
    """blob: bytes laid into the source buffer; src_len: how many of
    them the descriptor admits (the rest follow the slice directly, as
    the next page's bytes would); ulen: the descriptor's
    uncompressed_len; err: the code the kernel must report."""
    __slots__ = ("name", "blob", "src_len", "ulen", "mode", "err")

    def __init__(self, name, blob, src_len, ulen, mode, err):
        self.name, self.blob, self.src_len = name, bytes(blob), src_len
        self.ulen, self.mode, self.err = ulen, mode, err

    def __repr__(self):
        return "Refused(%s)" % self.name


@functools.lru_cache(maxsize=None)
def gzip_refused():
    P = payloads()
    out = []
    streams = {
        "dynamic": (TEXT, deflate(TEXT, 6, 0)),
        "fixed": (P["two"], deflate(P["two"], 6, zlib.Z_FIXED)),
        "stored": (P["random"], deflate(P["random"], 0, 0)),
        "flushed": (TEXT, deflate(TEXT, 6, zlib.Z_RLE, zlib.Z_FULL_FLUSH,
                                  len(TEXT) - 1)),
    }
    for kind, (p, raw) in streams.items():
        n = len(p)
        out.append(Refused("cut1-" + kind, raw, len(raw) - 1, n, 0, 1))
        out.append(Refused("half-" + kind, raw, len(raw) // 2, n, 0, 1))
        out.append(Refused("ulen-1-" + kind, raw, len(raw), n - 1, 0, 1))
        out.append(Refused("ulen+1-" + kind, raw, len(raw), n + 1, 0, 2))
        # wrapped: the 8-byte trailer is not part of the deflate data, so
        # cut it off and one byte more
        gz = gzip_wrap(raw, p, FNAME | FHCRC)
        out.append(Refused("gz-cut1-" + kind, gz, len(gz) - 9, n, 1, 1))
        out.append(Refused("gz-ulen-1-" + kind, gz, len(gz), n - 1, 1, 1))
        out.append(Refused("gz-ulen+1-" + kind, gz, len(gz), n + 1, 1, 2))
    p, raw = streams["dynamic"]
    out.append(Refused("reserved-block-type", b"\x07\x00\x00\x00", 4, 0,
                       0, 3))
    # a good non-final stored block, then block type 3
    two = b"\x00\x03\x00\xfc\xffabc" + b"\x07\x00"
    out.append(Refused("reserved-type-second-block", two, len(two), 3, 0,
                       3))
    gz = bytearray(gzip_wrap(raw, p))
    gz[1] = 0x8C
    out.append(Refused("gz-wrong-magic", gz, len(gz), len(p), 1, 3))
    gz = bytearray(gzip_wrap(raw, p))
    gz[2] = 7
    out.append(Refused("gz-method-7", gz, len(gz), len(p), 1, 3))
    out.append(Refused("gz-header-only", gzip_wrap(raw, p)[:10], 10,
                       len(p), 1, 1))
    out.append(Refused("gz-shorter-than-header", gzip_wrap(raw, p)[:9], 9,
                       len(p), 1, 3))
    sp, sraw = streams["stored"]
    bad = bytearray(sraw)
    assert bad[0] == 1 and bad[1] ^ bad[3] == 0xFF
    bad[3] ^= 0x10
    out.append(Refused("stored-nlen", bad, len(bad), len(sp), 0, 1))
    return tuple(out)


def _elements(ulen, *parts):
    return varint(ulen) + b"".join(parts)


_LIT8 = b"\x1c" + b"ABCDEFGH"              # literal, 8 bytes


def _c2(off, ln):
    return bytes([2 | ((ln - 1) << 2)]) + struct.pack("<H", off)


@functools.lru_cache(maxsize=None)
def snappy_refused():
    def whole(name, stream, ulen, err):
        return Refused(name, stream, len(stream), ulen, 0, err)
    return (
        whole("copy-offset-0", _elements(12, _LIT8, _c2(0, 4)), 12, 1),
        whole("copy1-offset-0", _elements(12, _LIT8, b"\x01\x00"), 12, 1),
        whole("copy-offset-past-start",
              _elements(12, _LIT8, _c2(9, 4)), 12, 1),
        whole("copy-first-element", _elements(4, _c2(1, 4)), 4, 1),
        whole("copy-overruns-output",
              _elements(12, _LIT8, _c2(4, 10)), 12, 1),
        whole("literal-overruns-output",
              _elements(12, _LIT8, _LIT8), 12, 1),
        whole("varint-larger", _elements(9, _LIT8, b"\x00Z"), 8, 2),
        whole("varint-smaller", _elements(8, _LIT8), 9, 2),
        whole("ends-early", _elements(20, _LIT8), 20, 1),
        whole("literal-cut-short", _elements(8, _LIT8)[:-1], 8, 1),
    )


@functools.lru_cache(maxsize=None)
def snappy_cut_operands():
    """Valid streams whose last element completes the output; src_len
    stops inside that element's operand bytes, which follow the slice
    directly in the buffer. (name, Refused, bytes the full stream
    decodes to)."""
    rng = np.random.default_rng(5)
    seed = rng.integers(0, 256, 16, dtype=np.uint8).tobytes()
    out = []
    for name, build, cut in (
            ("copy1", lambda s: s.copy1(16, 11), 1),
            ("copy2", lambda s: s.copy2(16, 16), 2),
            ("copy2-half", lambda s: s.copy2(16, 16), 1),
            ("copy4", lambda s: s.copy4(16, 16), 4),
            ("copy4-half", lambda s: s.copy4(16, 16), 2),
            ("literal-2-byte-length",
             lambda s: s.literal(bytes(range(200)), form=2), 202),
            ("literal-2-byte-length-half",
             lambda s: s.literal(bytes(range(200)), form=2), 201)):
        s = Snappy().literal(seed)
        build(s)
        st = s.stream()
        out.append((name, Refused("cut-" + name, st, len(st) - cut,
                                  len(s.out), 0, 1), s.expected()))
    return tuple(out)
