"""ops.DeviceStringDict (k_str_dict_encode, k_str_dict_rehash) driven
directly with the adversarial inputs of tests/_str_cases.py: strings whose
64-bit hashes are equal, raw hash 0 next to raw hash 1, a probe cluster that
wraps the table end, the length and tail edges of the hash and compare
loops, each growth condition of _ensure at its boundary, and the entry
edges of encode_column.

Reference: a Python dict on the same bytes. Code numbers inside a batch are
unordered (they come from an atomic counter), so the comparison is up to a
bijection: equal bytes <=> equal code, codes dense in [0, n_distinct), a
code once returned never changes, n_codes exact, and the stored bytes
(values_bytes) equal the input bytes. Every test that relies on the host
hash model stands on test_model_matches_device."""
import numpy as np
import pytest

import _str_cases as S

pa = pytest.importorskip("pyarrow")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from quokka_amd import shim
    shim.init(0)
    return shim


def _pack(strs):
    """list of bytes -> (offsets np.int64[n + 1], data np.uint8)."""
    offs = np.zeros(len(strs) + 1, dtype=np.int64)
    np.cumsum([len(b) for b in strs], out=offs[1:])
    return offs, np.frombuffer(b"".join(strs), dtype=np.uint8)


class _Ref:
    """The dict reference, carried across batches."""

    def __init__(self, sd):
        self.sd = sd
        self.code = {}

    def encode(self, strs):
        """Encode one batch and hold it against the reference."""
        codes = self.sd.encode(*_pack(strs))
        assert codes.dtype == np.uint32 and len(codes) == len(strs)
        taken = set(self.code.values())
        for b, c in zip(strs, codes.tolist()):
            if b in self.code:
                assert self.code[b] == c, b
            else:
                assert c not in taken, b
                taken.add(c)
                self.code[b] = c
        self.check()
        return codes

    def check(self):
        sd = self.sd
        assert sd.n_codes == len(self.code)
        assert sorted(self.code.values()) == list(range(len(self.code)))
        stored = sd.values_bytes
        assert len(stored) == len(self.code)
        for b, c in self.code.items():
            assert stored[c] == b, c
        assert sd.arena_used == sum(len(b) for b in self.code)

    def recheck_all(self):
        """Re-encode every string seen so far: old codes, nothing new."""
        n = self.sd.n_codes
        strs = list(self.code)
        if strs:
            self.encode(strs[::-1])
        assert self.sd.n_codes == n


def _slots(sd):
    return (sd.slot_hash.to_numpy(sd.cap).tolist(),
            sd.slot_code.to_numpy(sd.cap).tolist())


def _check_probe_invariant(sd, ref):
    """Every string's (hash, code) sits in a slot reachable from its home
    slot through occupied slots only, and nothing else is in the table."""
    sh, sc = _slots(sd)
    cap = sd.cap
    assert sorted(h for h in sh if h) == sorted(
        S.str_hash(b) for b in ref.code)
    for b, c in ref.code.items():
        s = S.home_slot(b, cap)
        for _ in range(cap):
            assert sh[s] != 0, (b, s)
            if sc[s] == c:
                break
            s = (s + 1) & (cap - 1)
        assert sc[s] == c and sh[s] == S.str_hash(b), b
    assert all(c == -1 for h, c in zip(sh, sc) if h == 0)


def _fillers(n, tag=b"fill"):
    return [b"%s-%06d" % (tag, i) for i in range(n)]


def test_model_matches_device(gpu):
    """The host hash model is the device's: after the edge table goes into
    a 64-slot dictionary, slot_hash holds exactly the model hashes, each at
    its home slot or the next free one after it."""
    from quokka_amd import ops
    sd = ops.DeviceStringDict(expected=16)
    assert sd.cap == 64
    ref = _Ref(sd)
    ref.encode(S.EDGES)
    assert sd.cap == 64 and sd.n_codes == len(S.EDGES)
    _check_probe_invariant(sd, ref)
    sd.free()


def test_exact_hash_collisions(gpu):
    """Four different strings with one 64-bit hash: four codes, the hash
    four times in consecutive slots, the same codes from a second batch in
    another order and after the table has grown."""
    from quokka_amd import ops, shim
    coll = S.colliding(24, 4, seed=11)
    h = S.str_hash(coll[0])
    n = 4 * shim.BLOCK_THREADS + 3
    rng = np.random.default_rng(2)
    sd = ops.DeviceStringDict(expected=16)
    ref = _Ref(sd)
    codes = ref.encode([coll[i] for i in rng.integers(0, 4, n)])
    assert sd.n_codes == 4 and len(set(codes.tolist())) == 4

    def run_of_four():
        sh, _ = _slots(sd)
        home = h & (sd.cap - 1)
        assert [sh[(home + j) & (sd.cap - 1)] for j in range(4)] == [h] * 4
        assert sum(1 for x in sh if x) == sd.n_codes
        _check_probe_invariant(sd, ref)

    run_of_four()
    ref.encode([coll[i] for i in rng.permutation(np.arange(n) % 4)])
    assert sd.n_codes == 4
    cap0 = sd.cap
    ref.encode(_fillers(cap0 // 2))              # forces a rehash
    assert sd.cap > cap0
    n_codes = sd.n_codes
    ref.encode([coll[i] for i in rng.integers(0, 4, n)])
    assert sd.n_codes == n_codes
    _check_probe_invariant(sd, ref)
    sh, _ = _slots(sd)
    assert sh.count(h) == 4
    sd.free()


def test_raw_hash_zero_next_to_one(gpu):
    """Raw hash 0 is stored as 1, the value a string of raw hash 1 stores
    too: two codes, slots 1 and 2, both holding 1."""
    from quokka_amd import ops
    zero, one = S.with_raw_hash(0, 16), S.with_raw_hash(1, 19)
    assert S.raw_hash(zero) == 0 and S.raw_hash(one) == 1
    sd = ops.DeviceStringDict(expected=16)
    ref = _Ref(sd)
    codes = ref.encode([zero, one, one, zero, zero, one])
    assert sd.cap == 64 and sd.n_codes == 2
    assert codes[0] != codes[1]
    sh, sc = _slots(sd)
    assert sh[1] == 1 and sh[2] == 1
    assert sorted(sc[1:3]) == [0, 1]
    assert sum(1 for x in sh if x) == 2
    ref.encode([one, zero])
    ref.encode(_fillers(200))
    assert sd.cap > 64
    ref.encode([zero, one, zero])
    _check_probe_invariant(sd, ref)
    sd.free()


def test_cluster_wraps_table_end(gpu):
    """Home slots 62, 63, 63, 63, 0 of a 64-slot table, inserted in one
    batch: the cluster runs over the end into slots 0, 1, 2. Found again
    in a later batch and after growth."""
    from quokka_amd import ops
    strs = S.home_slot_set(64, [62, 63, 63, 63, 0])
    sd = ops.DeviceStringDict(expected=16)
    ref = _Ref(sd)
    ref.encode(strs)
    assert sd.cap == 64
    sh, _ = _slots(sd)
    assert sorted(i for i, x in enumerate(sh) if x) == [0, 1, 2, 62, 63]
    _check_probe_invariant(sd, ref)
    ref.encode(strs[::-1] + strs + strs[2:4])      # 12 rows: no growth
    assert sd.cap == 64 and sd.n_codes == 5
    ref.encode(_fillers(100))
    assert sd.cap > 64
    ref.encode(strs[::-1])
    _check_probe_invariant(sd, ref)
    sd.free()


def test_edge_table_pairs_get_different_codes(gpu):
    """Prefixes, NUL-padded twins, zero words, embedded NULs, multi-byte
    UTF-8: every pair of different entries gets different codes, equal
    entries the same one."""
    from quokka_amd import ops
    sd = ops.DeviceStringDict(expected=16)
    ref = _Ref(sd)
    codes = ref.encode(S.EDGES + S.EDGES[::-1])
    n = len(S.EDGES)
    assert sd.n_codes == n
    first = codes[:n].tolist()
    assert len(set(first)) == n
    assert codes[n:].tolist() == first[::-1]
    assert sd.values == [b.decode() for b in sd.values_bytes]
    sd.free()


def _rows_table_at():
    """Rows after which 2 * need == cap: the slot table's boundary."""
    return _fillers(32), [b"one-more"]


def _rows_codes_at():
    """Rows after which need == code_cap (1024 code_off/code_len)."""
    return _fillers(1024), [b"one-more"]


def _rows_arena_at():
    """Rows summing to exactly 1 << 20 arena bytes, then one byte."""
    rows = [(b"%04d" % i) * 256 for i in range(1024)]
    assert sum(len(b) for b in rows) == 1 << 20
    return rows, [b"x"]


def _caps(sd):
    return {"table": sd.cap, "codes": sd.code_cap, "arena": sd.arena_cap}


@pytest.mark.parametrize("which,rows", [("table", _rows_table_at),
                                        ("codes", _rows_codes_at),
                                        ("arena", _rows_arena_at)],
                         ids=["table", "codes", "arena"])
def test_growth_boundaries(gpu, which, rows):
    """Each _ensure condition exactly at its boundary (no growth), one
    row or byte past it in a later batch (growth), and one past it in a
    single batch. Codes, bytes and n_codes survive every step."""
    from quokka_amd import ops
    at, more = rows()
    # at the boundary: nothing grows, everything is found again
    sd = ops.DeviceStringDict(expected=16)
    before = _caps(sd)
    ref = _Ref(sd)
    ref.encode(at)
    assert _caps(sd)[which] == before[which]
    if which == "table":
        assert 2 * sd.n_codes == sd.cap
    elif which == "codes":
        assert sd.n_codes == sd.code_cap
    else:
        assert sd.arena_used == sd.arena_cap == 1 << 20
    ref.recheck_all()
    sd.free()
    # one past it in the next batch
    sd = ops.DeviceStringDict(expected=16)
    ref = _Ref(sd)
    ref.encode(at)
    assert _caps(sd)[which] == before[which]
    ref.encode(more)
    assert _caps(sd)[which] > before[which]
    ref.recheck_all()
    sd.free()
    # one past it within one batch
    sd = ops.DeviceStringDict(expected=16)
    ref = _Ref(sd)
    ref.encode(at + more)
    assert _caps(sd)[which] > before[which]
    ref.recheck_all()
    sd.free()


def test_growth_all_three_at_once(gpu):
    """One batch that grows the slot table, the code arrays and the arena
    together, over a dictionary that already holds strings."""
    from quokka_amd import ops
    sd = ops.DeviceStringDict(expected=16)
    ref = _Ref(sd)
    ref.encode(S.EDGES + S.colliding(16, 3, seed=5))
    before = _caps(sd)
    ref.encode([(b"%05d" % i) * 200 for i in range(1100)])
    after = _caps(sd)
    assert all(after[k] > before[k] for k in before), (before, after)
    ref.recheck_all()
    _check_probe_invariant(sd, ref)
    sd.free()


def test_one_string_many_copies(gpu):
    """4096 copies of one 33-byte string: one code, 33 arena bytes (only
    the lane that claims the slot copies the string in)."""
    from quokka_amd import ops
    s = b"the-same-thirty-three-byte-string"
    assert len(s) == 33
    sd = ops.DeviceStringDict(expected=16)
    ref = _Ref(sd)
    codes = ref.encode([s] * 4096)
    assert not codes.any()
    assert sd.n_codes == 1 and sd.arena_used == 33
    assert sd.values_bytes == [s]
    sd.free()


# ---- encode_column ------------------------------------------------------

def _check_column(sd, col, want):
    """encode_column(col) against the dict reference on `want` (str)."""
    codes = sd.encode_column(col)
    vals = sd.values
    assert [vals[c] for c in codes.tolist()] == want
    assert len(set(codes.tolist())) == len(set(want))
    return codes


@pytest.mark.parametrize("typ", ["string", "large_string"])
def test_encode_column_sliced(gpu, typ):
    """A slice with a non-zero offset reads its own rows, in both offset
    widths."""
    from quokka_amd import ops
    strs = [b.decode() for b in S.EDGES] + ["s%d" % (i % 7) for i in range(40)]
    arr = pa.array(strs, type=getattr(pa, typ)())
    sd = ops.DeviceStringDict(expected=16)
    seen = set()
    for lo, ln in ((3, 10), (0, 5), (17, 30), (len(strs) - 1, 1)):
        sl = arr.slice(lo, ln)
        assert sl.offset == lo
        _check_column(sd, sl, strs[lo:lo + ln])
        _check_column(sd, pa.chunked_array([sl]), strs[lo:lo + ln])
        seen.update(strs[lo:lo + ln])
        assert sd.n_codes == len(seen)
    sd.free()


def test_encode_column_dictionary_two_chunks(gpu):
    from quokka_amd import ops
    a = ["x", "yy", "x", "", "zzz"]
    b = ["yy", "q", "q", "x"]
    col = pa.chunked_array([pa.array(a).dictionary_encode(),
                            pa.array(b).dictionary_encode()])
    assert pa.types.is_dictionary(col.type) and col.num_chunks == 2
    sd = ops.DeviceStringDict(expected=16)
    codes = _check_column(sd, col, a + b)
    assert codes[0] == codes[2] == codes[8] and codes[1] == codes[5]
    assert sd.n_codes == 5
    sd.free()


def test_encode_column_only_empty_strings(gpu):
    """A column of nothing but empty strings: no data bytes at all, or
    none that its rows cover."""
    from quokka_amd import ops
    sd = ops.DeviceStringDict(expected=16)
    codes = _check_column(sd, pa.array(["", "", ""]), ["", "", ""])
    assert codes.tolist() == [0, 0, 0]
    sliced = pa.array(["abc", "", "", ""]).slice(1)
    assert sd.encode_column(sliced).tolist() == [0, 0, 0]
    large = pa.array(["", ""], type=pa.large_string())
    assert sd.encode_column(large).tolist() == [0, 0]
    assert sd.n_codes == 1 and sd.arena_used == 0
    assert sd.values_bytes == [b""]
    sd.free()


def test_encode_column_null_slot_over_bytes(gpu):
    """nulls="mask": a null slot whose offsets cover real bytes. The mask
    says which rows count; the valid rows' codes are those the same
    strings get without the null beside them."""
    from quokka_amd import ops
    offs = np.array([0, 2, 5, 7, 7], dtype=np.int32)
    col = pa.Array.from_buffers(
        pa.string(), 4,
        [pa.py_buffer(np.array([0b1101], dtype=np.uint8)),
         pa.py_buffer(offs), pa.py_buffer(b"aaXXXbb")])
    assert col.to_pylist() == ["aa", None, "bb", ""]
    sd = ops.DeviceStringDict(expected=16)
    with pytest.raises(TypeError, match="null"):
        sd.encode_column(col)
    codes, mask = sd.encode_column(col, nulls="mask")
    assert mask.dtype == bool and mask.tolist() == [True, False, True, True]
    stored = sd.values_bytes
    assert [stored[c] for c in codes[mask].tolist()] == [b"aa", b"bb", b""]
    plain = sd.encode_column(pa.array(["bb", "", "aa"]))
    assert plain.tolist() == [codes[2], codes[3], codes[0]]
    codes2, mask2 = sd.encode_column(pa.array(["aa", "bb"]), nulls="mask")
    assert mask2 is None and codes2.tolist() == [codes[0], codes[2]]
    sd.free()


def test_encode_column_utf8_round_trip(gpu):
    from quokka_amd import ops
    strs = ["\u00e9", "e\u0301", "\u65e5\u672c", "\u65e5\u672c\u8a9e",
            "\U0001F600", "na\u00efve caf\u00e9", "\u00e9"]
    sd = ops.DeviceStringDict(expected=16)
    codes = _check_column(sd, pa.array(strs), strs)
    assert codes[0] == codes[6] and codes[0] != codes[1]
    assert sd.decode(codes).tolist() == strs
    assert sd.values_bytes == [s.encode() for s in sd.values]
    sd.free()


@pytest.mark.parametrize("make,name", [
    (lambda: pa.array([b"ab", b"c"], type=pa.binary()), "binary"),
    (lambda: pa.array([b"ab", b"c"], type=pa.large_binary()),
     "large_binary"),
    (lambda: pa.array([1, 2, 3], type=pa.int64()), "int64"),
    (lambda: pa.array([1.5, 2.5]), "double"),
    (lambda: pa.chunked_array([pa.array([b"ab"], type=pa.large_binary())]),
     "large_binary"),
    (lambda: pa.array([1, 2, 1]).dictionary_encode(), "int64"),
], ids=["binary", "large_binary", "int64", "double", "chunked_large_binary",
        "dictionary_of_int64"])
def test_encode_column_refuses_non_strings(gpu, make, name):
    """Anything but string / large_string (or a dictionary of them) is
    refused by name, not read with some offset width."""
    from quokka_amd import ops
    sd = ops.DeviceStringDict(expected=16)
    with pytest.raises(TypeError, match=name):
        sd.encode_column(make())
    with pytest.raises(TypeError, match=name):
        sd.encode_column(make(), nulls="mask")
    assert sd.n_codes == 0
    sd.free()
