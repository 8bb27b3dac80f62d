"""The builders of tests/_str_cases.py keep their promises under the host
model of the string hash, so a GPU test built on them tests what it says
(tests/test_gpu_str_dict.py checks model == device). No GPU."""
import random
from collections import Counter

import pytest

import _str_cases as S


def test_splitmix64_known_vector_and_inverse():
    assert S.splitmix64(0) == 0xE220A8397B1DCDAF      # canonical, seed 0
    rng = random.Random(1)
    xs = [0, 1, 2 ** 63, 2 ** 64 - 1] + [rng.getrandbits(64)
                                         for _ in range(1000)]
    for x in xs:
        assert S.unsplitmix64(S.splitmix64(x)) == x
        assert S.splitmix64(S.unsplitmix64(x)) == x


def test_str_hash_structure():
    """Length in the seed, little-endian tail packing, one closing round
    even when the tail is empty, and the 0 -> 1 remap."""
    g = S.GOLDEN
    assert S.raw_hash(b"") == S.splitmix64(g)
    assert S.raw_hash(b"a") == S.splitmix64(g ^ 1 ^ 0x61)
    assert S.raw_hash(b"ab") == S.splitmix64(g ^ 2 ^ 0x6261)
    w = int.from_bytes(b"abcdefgh", "little")
    assert S.raw_hash(b"abcdefgh") == S.splitmix64(S.splitmix64(g ^ 8 ^ w))
    assert S.raw_hash(b"abcdefghi") == S.splitmix64(
        S.splitmix64(g ^ 9 ^ w) ^ 0x69)
    # the same padded tail word, told apart by the length alone
    assert len({S.str_hash(b"a"), S.str_hash(b"a\0"),
                S.str_hash(b"a\0\0")}) == 3
    assert S.str_hash(b"\0" * 8) != S.str_hash(b"\0" * 16)


@pytest.mark.parametrize("length,k,seed", [(16, 2, 0), (16, 4, 1),
                                           (24, 4, 2), (29, 6, 3),
                                           (40, 3, 4)])
def test_colliding_strings(length, k, seed):
    c = S.colliding(length, k, seed)
    assert len(c) == k and len(set(c)) == k
    assert all(len(b) == length for b in c)
    assert len({S.str_hash(b) for b in c}) == 1
    assert S.str_hash(c[0]) == S.raw_hash(c[0])      # not the remapped 0
    for b in c:
        assert b.decode().encode() == b               # valid UTF-8
    assert S.colliding(length, k, seed) == c          # deterministic
    with pytest.raises(ValueError):
        S.colliding(15, 2)


@pytest.mark.parametrize("length", [8, 9, 15, 16, 17, 31, 32])
def test_with_raw_hash(length):
    rng = random.Random(length)
    for target in (0, 1, 2 ** 64 - 1, rng.getrandbits(64)):
        b = S.with_raw_hash(target, length)
        assert len(b) == length and S.raw_hash(b) == target
    zero, one = S.with_raw_hash(0, length), S.with_raw_hash(1, length)
    assert zero != one
    assert S.str_hash(zero) == 1 == S.str_hash(one)   # share a stored value


def test_home_slot_set():
    want = [62, 63, 63, 63, 0]
    got = S.home_slot_set(64, want)
    assert len(set(got)) == len(want)
    assert [S.home_slot(b, 64) for b in got] == want
    other = S.home_slot_set(64, want, seed=1)
    assert [S.home_slot(b, 64) for b in other] == want
    assert not set(other) & set(got)
    assert [S.home_slot(b, 1024) for b in
            S.home_slot_set(1024, [1023, 1023, 0])] == [1023, 1023, 0]


def test_edge_table():
    assert len(set(S.EDGES)) == len(S.EDGES)
    # fits a 64-slot table without growth (the table keeps 2 * rows <= cap)
    assert 2 * len(S.EDGES) <= 64
    assert {0, 1, 7, 8, 9, 15, 16, 17} <= {len(b) for b in S.EDGES}
    for b in S.EDGES:
        assert b.decode().encode() == b
    # no two edges collide, so model == device can compare hash multisets
    assert len({S.str_hash(b) for b in S.EDGES}) == len(S.EDGES)
    for a in (b"a", b"a\0", b"a\0\0", b"\0" * 8, b"\0" * 16):
        assert a in S.EDGES
    assert any(x != y and y.startswith(x) for x in S.EDGES for y in S.EDGES)


def test_channel_of_rule_and_partition_key_set():
    for b in S.EDGES:
        for n in (1, 2, 3, 4, 7):
            assert S.channel_of(b, n) == (S.str_hash(b) >> 1) % n
            assert 0 <= S.channel_of(b, n) < n
    keys = S.partition_keys()
    assert len(keys) == 512 == len(set(keys))
    assert S.partition_keys() == keys
    per = Counter(S.channel_of(k, S.PARTITION_N) for k in keys)
    # a condition on the inputs of the GPU partition test: every channel
    # gets keys, so an empty output channel there is a lost channel
    assert sorted(per) == list(range(S.PARTITION_N))
    assert min(per.values()) >= 64
