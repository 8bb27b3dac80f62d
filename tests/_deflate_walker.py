"""Pure-Python DEFLATE walker (RFC 1951), written from the RFC text alone.

Test helper, not product code: it shares no table, constant or routine
with the GPU decoder (quokka_amd/csrc k_gzip_pages). It inflates a raw
deflate stream and reports WHICH parts of the format the stream uses, so
that (a) it is a second CPU reference beside zlib and (b) every GPU test
can assert that its input really reaches the decoder path the test is
named for.

Bits are addressed by absolute position (bit k of the stream is bit k&7
of byte k>>3), so byte alignment before a stored block is plain
arithmetic on the position, with no buffered state to resynchronise.
"""


class Walk:
    """Result of walk(): output bytes plus per-stream statistics."""
    __slots__ = ("data", "blocks", "max_lit_bits", "max_dist_bits",
                 "max_len", "max_dist", "end_bit")

    def __init__(self):
        self.data = b""
        self.blocks = []        # "stored" | "fixed" | "dynamic", in order
        self.max_lit_bits = 0   # longest literal/length code DECODED
        self.max_dist_bits = 0  # longest distance code DECODED
        self.max_len = 0        # longest match
        self.max_dist = 0       # farthest match
        self.end_bit = 0        # bit position after the final block

    def huffman_then_stored(self):
        """True if a stored block directly follows a Huffman block."""
        b = self.blocks
        return any(b[i] != "stored" and b[i + 1] == "stored"
                   for i in range(len(b) - 1))


def _length_table():
    # RFC 1951 3.2.5: codes 257..264 are lengths 3..10 with no extra
    # bits, then groups of four codes share 1, 2, .. 5 extra bits; 285
    # is length 258 with none.
    tab = {}
    base = 3
    for code in range(257, 285):
        extra = 0 if code < 265 else (code - 261) // 4
        tab[code] = (base, extra)
        base += 1 << extra
    tab[285] = (258, 0)
    return tab


def _dist_table():
    # codes 0..3 are distances 1..4, then pairs of codes share 1..13
    # extra bits
    tab = {}
    base = 1
    for code in range(30):
        extra = 0 if code < 4 else (code - 2) // 2
        tab[code] = (base, extra)
        base += 1 << extra
    return tab


_LENGTHS = _length_table()
_DISTS = _dist_table()
_CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1,
             15)


def _canonical(lengths):
    """RFC 1951 3.2.2: code lengths -> {(1 << len) | code: symbol}."""
    bl_count = [0] * 16
    for ln in lengths:
        bl_count[ln] += 1
    bl_count[0] = 0
    next_code = [0] * 16
    code = 0
    for bits in range(1, 16):
        code = (code + bl_count[bits - 1]) << 1
        next_code[bits] = code
    left = 1
    for bits in range(1, 16):
        left = (left << 1) - bl_count[bits]
        if left < 0:
            raise ValueError("over-subscribed code")
    table = {}
    for sym, ln in enumerate(lengths):
        if ln:
            table[(1 << ln) | next_code[ln]] = sym
            next_code[ln] += 1
    return table


_FIXED_LIT = _canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
_FIXED_DIST = _canonical([5] * 30)


class _Bits:
    def __init__(self, data):
        self.data = data
        self.nbits = 8 * len(data)
        self.pos = 0

    def take(self, n):
        """n <= 16 data bits, least significant bit first."""
        if n == 0:
            return 0
        pos = self.pos
        if pos + n > self.nbits:
            raise ValueError("stream ends inside a field")
        byte = pos >> 3
        v = int.from_bytes(self.data[byte:byte + 4], "little")
        self.pos = pos + n
        return (v >> (pos & 7)) & ((1 << n) - 1)

    def symbol(self, table):
        """One Huffman code, most significant code bit first.
        Returns (symbol, code length)."""
        pos = self.pos
        byte = pos >> 3
        window = int.from_bytes(self.data[byte:byte + 4], "little") \
            >> (pos & 7)
        avail = self.nbits - pos
        code = 1
        for ln in range(1, 16):
            if ln > avail:
                raise ValueError("stream ends inside a code")
            code = (code << 1) | (window & 1)
            window >>= 1
            sym = table.get(code)
            if sym is not None:
                self.pos = pos + ln
                return sym, ln
        raise ValueError("bit pattern is no code")


def _dynamic_tables(br):
    hlit = br.take(5) + 257
    hdist = br.take(5) + 1
    hclen = br.take(4) + 4
    if hlit > 286 or hdist > 30:
        raise ValueError("too many codes")
    cl = [0] * 19
    for i in range(hclen):
        cl[_CL_ORDER[i]] = br.take(3)
    cl_table = _canonical(cl)
    lengths = []
    while len(lengths) < hlit + hdist:
        sym, _ = br.symbol(cl_table)
        if sym < 16:
            lengths.append(sym)
        elif sym == 16:
            if not lengths:
                raise ValueError("repeat with nothing before it")
            lengths.extend([lengths[-1]] * (3 + br.take(2)))
        elif sym == 17:
            lengths.extend([0] * (3 + br.take(3)))
        else:
            lengths.extend([0] * (11 + br.take(7)))
    if len(lengths) > hlit + hdist:
        raise ValueError("code lengths overrun")
    if lengths[256] == 0:
        raise ValueError("no end-of-block code")
    return _canonical(lengths[:hlit]), _canonical(lengths[hlit:])


def walk(stream):
    """Inflate a raw deflate stream; raise ValueError if it is invalid."""
    br = _Bits(bytes(stream))
    out = bytearray()
    res = Walk()
    final = 0
    while not final:
        final = br.take(1)
        btype = br.take(2)
        if btype == 0:
            res.blocks.append("stored")
            br.pos = (br.pos + 7) & ~7
            ln = br.take(16)
            nln = br.take(16)
            if ln ^ nln != 0xFFFF:
                raise ValueError("stored length check")
            start = br.pos >> 3
            if start + ln > len(br.data):
                raise ValueError("stored block cut short")
            out += br.data[start:start + ln]
            br.pos += 8 * ln
            continue
        if btype == 1:
            res.blocks.append("fixed")
            lit, dist = _FIXED_LIT, _FIXED_DIST
        elif btype == 2:
            res.blocks.append("dynamic")
            lit, dist = _dynamic_tables(br)
        else:
            raise ValueError("reserved block type")
        while True:
            sym, nb = br.symbol(lit)
            if nb > res.max_lit_bits:
                res.max_lit_bits = nb
            if sym < 256:
                out.append(sym)
                continue
            if sym == 256:
                break
            if sym > 285:
                raise ValueError("length code out of range")
            base, extra = _LENGTHS[sym]
            length = base + br.take(extra)
            dsym, nb = br.symbol(dist)
            if nb > res.max_dist_bits:
                res.max_dist_bits = nb
            if dsym > 29:
                raise ValueError("distance code out of range")
            base, extra = _DISTS[dsym]
            distance = base + br.take(extra)
            if distance > len(out):
                raise ValueError("distance before start of output")
            if length > res.max_len:
                res.max_len = length
            if distance > res.max_dist:
                res.max_dist = distance
            if distance >= length:
                s = len(out) - distance
                out += out[s:s + length]
            else:
                for _ in range(length):
                    out.append(out[-distance])
    res.data = bytes(out)
    res.end_bit = br.pos
    return res
