"""Host model of the device string hash (qk_str_hash in
quokka_amd/csrc/quokka_amd.hip) and builders of the inputs that the string
dictionary can get wrong without a random test noticing: different strings
whose 64-bit hashes are equal, strings of raw hash 0 and 1 (0 is stored as
1), strings with chosen home slots, and the length and tail edges of the
hash and compare loops. Plain Python, no GPU; tests/test_str_cases_cpu.py
checks what the builders promise, tests/test_gpu_str_dict.py checks that
this model and the device agree before it relies on either.

splitmix64 is a bijection on 64-bit words, so the hash, which folds it over
the string's 8-byte words, can be steered: whatever the state is before a
word, that word can be chosen to give any state after it."""
import random

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
_C1 = 0xBF58476D1CE4E5B9
_C2 = 0x94D049BB133111EB
_C1_INV = pow(_C1, -1, 1 << 64)
_C2_INV = pow(_C2, -1, 1 << 64)
_HIGH_BITS = 0x8080808080808080


def splitmix64(x):
    x = (x + GOLDEN) & M64
    x ^= x >> 30
    x = (x * _C1) & M64
    x ^= x >> 27
    x = (x * _C2) & M64
    x ^= x >> 31
    return x


def unsplitmix64(y):
    """The inverse: x ^= x >> s is undone by xoring in the shifts by s, 2s,
    ... below 64; the odd multipliers have inverses mod 2**64."""
    y ^= y >> 31
    y ^= y >> 62
    y = (y * _C2_INV) & M64
    y ^= y >> 27
    y ^= y >> 54
    y = (y * _C1_INV) & M64
    y ^= y >> 30
    y ^= y >> 60
    return (y - GOLDEN) & M64


def raw_hash(b):
    """qk_str_hash before its last line: seed = golden ^ length, one
    splitmix64 per whole little-endian 8-byte word, then one more over the
    zero-padded tail (a zero word when the length is a multiple of 8)."""
    b = bytes(b)
    h = GOLDEN ^ len(b)
    i = 0
    while i + 8 <= len(b):
        h = splitmix64(h ^ int.from_bytes(b[i:i + 8], "little"))
        i += 8
    return splitmix64(h ^ int.from_bytes(b[i:], "little"))


def str_hash(b):
    """qk_str_hash: 0 marks an empty slot, so a raw 0 is stored as 1."""
    return raw_hash(b) or 1


def home_slot(b, cap):
    return str_hash(b) & (cap - 1)


def channel_of(b, nparts):
    """The channel string hash partitioning sends `b` to: the top 63 bits
    of the hash as a non-negative integer, modulo the channel count
    (DESIGN.md §3a). The same in every call, process and rank."""
    return (str_hash(b) >> 1) % nparts


def _ascii_word(i):
    """8 lower-case letters that spell the number i in base 26."""
    out = bytearray(8)
    for k in range(8):
        out[k] = 97 + i % 26
        i //= 26
    return bytes(out)


def colliding(length, k, seed=0):
    """k pairwise different byte strings of `length` >= 16 bytes whose
    hashes are equal in all 64 bits. They differ in their first word; the
    second word of each cancels the difference (w2 = state ^ c for one
    common c), and from there on they are the same. First words are taken
    by counting upwards until the second word has every byte below 0x80,
    one candidate in 256, so each string is valid UTF-8 (control bytes
    included) and can travel in an Arrow string column."""
    if length < 16:
        raise ValueError("colliding: length must be >= 16")
    if k < 1:
        raise ValueError("colliding: k must be >= 1")
    rng = random.Random(seed)
    h0 = GOLDEN ^ length
    rest = bytes(rng.randrange(97, 123) for _ in range(length - 16))
    i = rng.randrange(26 ** 7)
    w1 = _ascii_word(i)
    w2 = _ascii_word(rng.randrange(26 ** 7))
    c = splitmix64(h0 ^ int.from_bytes(w1, "little")) \
        ^ int.from_bytes(w2, "little")
    out = [w1 + w2 + rest]
    while len(out) < k:
        i += 1
        w1 = _ascii_word(i)
        w2 = splitmix64(h0 ^ int.from_bytes(w1, "little")) ^ c
        if w2 & _HIGH_BITS:
            continue
        out.append(w1 + w2.to_bytes(8, "little") + rest)
    return out


def with_raw_hash(target, length, seed=0):
    """A byte string of `length` >= 8 whose raw hash is `target`: all of
    it is arbitrary but the last whole word, which is solved for. (Its
    bytes are whatever they come out as, not UTF-8.)"""
    if length < 8:
        raise ValueError("with_raw_hash: length must be >= 8")
    rng = random.Random(seed)
    nwords, ntail = divmod(length, 8)
    head = bytes(rng.randrange(97, 123) for _ in range(8 * (nwords - 1)))
    tail = bytes(rng.randrange(97, 123) for _ in range(ntail))
    h = GOLDEN ^ length
    for i in range(0, len(head), 8):
        h = splitmix64(h ^ int.from_bytes(head[i:i + 8], "little"))
    after = unsplitmix64(target & M64) ^ int.from_bytes(tail, "little")
    word = unsplitmix64(after) ^ h
    return head + word.to_bytes(8, "little") + tail


def home_slot_set(cap, slots, seed=0):
    """Distinct strings whose home slots in a table of `cap` slots are
    `slots`, in that order (a slot may repeat): found by counting upwards
    through the model."""
    want = list(slots)
    out = [None] * len(want)
    left = len(want)
    i = seed * 1_000_003
    while left:
        s = b"slot-%d" % i
        i += 1
        hs = home_slot(s, cap)
        for j, w in enumerate(want):
            if out[j] is None and w == hs:
                out[j] = s
                left -= 1
                break
    return out


_ALPHA = b"abcdefghijklmnopq"

# Lengths and tails at which the hash and compare loops change path. Every
# entry is valid UTF-8 (NUL is), and all are different.
EDGES = [
    b"",                                  # no word, zero tail
    b"a", b"a\0", b"a\0\0",               # same padded tail word, the
    b"\0",                                # length in the seed separates
    _ALPHA[:7], _ALPHA[:8], _ALPHA[:9],   # prefixes of each other, around
    _ALPHA[:15], _ALPHA[:16], _ALPHA[:17],  # one and two whole words
    b"\0" * 7, b"\0" * 8, b"\0" * 16,     # all-zero words
    b"ab\0cd", b"ab\0ce",                 # differ behind an embedded NUL
    "\u00e9".encode(), "e\u0301".encode(),   # one glyph, two spellings
    "\u65e5\u672c".encode(), "\u65e5\u672c\u8a9e".encode(),
    "\U0001F600".encode(),
]

PARTITION_N = 4
PARTITION_SEED = 7


def partition_keys(n=512, seed=PARTITION_SEED):
    """The n distinct keys of the cross-call partition test: ASCII, 3 to
    26 bytes long, so that whole-word, tail-only and mixed strings all
    occur. test_str_cases_cpu pins that no channel of PARTITION_N stays
    empty under channel_of."""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        pad = "".join(chr(rng.randrange(97, 123))
                      for _ in range(rng.randrange(0, 20)))
        out.append(("k%d-%s" % (i, pad)).encode())
    return out

