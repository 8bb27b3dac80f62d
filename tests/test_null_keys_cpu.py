"""Null keys without a GPU: the numpy model of tests/_null_key_cases.py
(key words + null words, the join rules) against pyarrow Acero, the
independent oracle (Table.group_by makes one group of null keys per null
pattern; Table.join never matches a null key), and the host half of the
executors: _KeyWords(null_keys=True) words, masks and the way back to
Arrow."""
import numpy as np
import pytest

import _null_key_cases as C

pa = pytest.importorskip("pyarrow")


def _arrow(col, mask):
    return pa.array(col) if mask is None else pa.array(col, mask=~mask)


@pytest.mark.parametrize("name", sorted(C.GROUP_CASES))
def test_model_groups_like_acero(name):
    cols, masks = C.GROUP_CASES[name]
    names = ["k%d" % i for i in range(len(cols))]
    t = pa.table({nm: _arrow(c, m) for nm, c, m in zip(names, cols, masks)})
    t = t.append_column("row", pa.array(np.arange(len(cols[0]))))
    want = t.group_by(names, use_threads=False).aggregate([("row", "list")])
    codes, seen = C.first_seen_codes(C.key_rows(cols, masks))
    assert len(seen) == want.num_rows
    got = {}
    for r, c in enumerate(codes.tolist()):
        got.setdefault(c, []).append(r)
    assert sorted(map(tuple, got.values())) == \
        sorted(tuple(sorted(g)) for g in want.column("row_list").to_pylist())


def test_model_four_tuples_are_four_keys():
    cols, masks = C.GROUP_CASES["four_tuples"]
    codes, seen = C.first_seen_codes(C.key_rows(cols, masks))
    assert len(seen) == 4
    assert codes.tolist() == [0, 1, 2, 3, 0, 1, 2, 3]
    canon, nullw = C.null_words(cols, masks)
    assert canon[0].tolist() == [0] * 8 and canon[1].tolist() == [0] * 8
    assert nullw[0].tolist() == [1, 2, 0, 3, 1, 2, 0, 3]


def test_model_null_words_two_words():
    """K = 65: key 64 lands in bit 0 of the second null word."""
    cols, masks = C.null_word_case(65, 65)
    canon, nullw = C.null_words(cols, masks)
    assert len(nullw) == 2
    assert np.array_equal(nullw[1] & 1, (~masks[64]).astype(np.int64))
    assert not (nullw[1] >> 1).any()
    for k in (1, 5):
        assert masks[k] is None and canon[k] is None
        assert not ((nullw[0] >> k) & 1).any()
    assert ((nullw[0] >> 2) & 1).all()                 # the all-null column
    assert not ((nullw[0] >> 3) & 1).any()             # the all-valid one
    bitmap, nulls = C.nullword_to_valid(nullw[1], 0, 65)
    assert len(bitmap) == C.valid_nbytes(65)
    assert nulls == int((~masks[64]).sum())
    assert np.array_equal(
        np.unpackbits(bitmap, bitorder="little")[:65].astype(bool), masks[64])
    assert not np.unpackbits(bitmap, bitorder="little")[65:].any()


_ACERO_JOIN = {0: "inner", 1: "left semi", 2: "left anti"}


@pytest.mark.parametrize("n_probe", C.JOIN_N_PROBE)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_model_joins_like_acero(n_probe, mode):
    builds, (pk, pm) = C.join_case(n_probe)
    bk = np.concatenate([k for k, _ in builds])
    bm = np.concatenate([m for _, m in builds])
    left = pa.table({"k": _arrow(pk, pm), "p": np.arange(len(pk))})
    right = pa.table({"k": _arrow(bk, bm), "b": np.arange(len(bk))})
    want = left.join(right, "k", join_type=_ACERO_JOIN[mode],
                     use_threads=False)
    got = C.join(bk, bm, pk, pm, mode)
    if mode == 0:
        assert sorted(zip(want.column("p").to_pylist(),
                          want.column("b").to_pylist())) == got
    else:
        assert sorted(want.column("p").to_pylist()) == got
    if mode == 2:       # anti keeps every null-key probe row
        assert set(np.nonzero(~pm)[0].tolist()) <= set(got)


def test_model_left_outer_keeps_null_probe_rows_like_acero():
    builds, (pk, pm) = C.join_case(65)
    bk = np.concatenate([k for k, _ in builds])
    bm = np.concatenate([m for _, m in builds])
    left = pa.table({"k": _arrow(pk, pm), "p": np.arange(len(pk))})
    right = pa.table({"k": _arrow(bk, bm), "b": np.arange(len(bk))})
    want = left.join(right, "k", join_type="left outer", use_threads=False)
    pairs = C.join(bk, bm, pk, pm, 0)
    unmatched = C.join(bk, bm, pk, pm, 2)
    rows = sorted(pairs + [(p, None) for p in unmatched],
                  key=lambda r: (r[0], -1 if r[1] is None else r[1]))
    got = sorted(zip(want.column("p").to_pylist(),
                     want.column("b").to_pylist()),
                 key=lambda r: (r[0], -1 if r[1] is None else r[1]))
    assert got == rows


# ---- _KeyWords(null_keys=True): host only --------------------------------
class _NoDeviceDict:
    """Stands in for ops.DeviceStringDict on a host without a GPU: the
    same encode_column(col, nulls=) contract over a Python dict."""

    def __init__(self, expected=0):
        self.codes = {}
        self.values = []

    def encode_column(self, col, stream=None, nulls="raise"):
        import pyarrow.compute as pc
        if isinstance(col, pa.ChunkedArray):
            col = col.combine_chunks()
        if pa.types.is_dictionary(col.type):
            col = col.cast(col.type.value_type)
        if col.null_count and nulls == "raise":
            raise TypeError("null string keys unsupported")
        out = np.empty(len(col), dtype=np.uint32)
        for i, v in enumerate(col.to_pylist()):
            v = "" if v is None else v     # a null covers no bytes
            if v not in self.codes:
                self.codes[v] = len(self.values)
                self.values.append(v)
            out[i] = self.codes[v]
        if nulls != "mask":
            return out
        mask = pc.is_valid(col).to_numpy(zero_copy_only=False) \
            if col.null_count else None
        return out, mask

    def decode(self, codes):
        return np.asarray(self.values, dtype=object)[
            np.asarray(codes, dtype=np.int64)]

    def free(self):
        pass


class _NoDeviceOps:
    DeviceStringDict = _NoDeviceDict


def _key_words():
    from quokka_amd.executors import _KeyWords
    return _KeyWords


_ROUND_TRIP = {
    "int32": pa.array([5, None, -7, None, 0], type=pa.int32()),
    "int64": pa.array([1 << 40, None, C.I64_MIN, None, 0], type=pa.int64()),
    "uint64": pa.array([2 ** 64 - 1, None, 0, None, 7], type=pa.uint64()),
    "bool": pa.array([True, None, False, None, True]),
    "date32": pa.array([8035, None, 0, None, -1], type=pa.int32()
                       ).cast(pa.date32()),
    "timestamp": pa.array([10 ** 15, None, 0, None, -5], type=pa.int64()
                          ).cast(pa.timestamp("us")),
    "float32": pa.array([1.5, None, -2.25, None, 0.0], type=pa.float32()),
    "float64": pa.array([1e300, None, -0.5, None, 3.0], type=pa.float64()),
    "string": pa.array(["a", None, "", None, "bc"]),
    "dict_string": pa.array(["x", None, "y", None, "x"]
                            ).dictionary_encode(),
}


@pytest.mark.parametrize("name", sorted(_ROUND_TRIP))
def test_key_words_round_trip_keeps_type_and_nulls(name):
    col = _ROUND_TRIP[name]
    kw = _key_words()(["k"], null_keys=True)
    kw.check(pa.table({"k": col}), "test")          # accepts nulls
    words, masks = kw.words(pa.table({"k": col}), _NoDeviceOps)
    assert words[0].dtype == np.int64
    assert masks[0].tolist() == [True, False, True, False, True]
    assert words[0][~masks[0]].tolist() == [0, 0], "0 under every null"
    back = kw.to_arrow("k", kw.decode("k", words[0], masks[0]), masks[0])
    # a dictionary-encoded key comes back in its value type, as it does
    # on the path without nulls
    want_type = col.type.value_type if pa.types.is_dictionary(col.type) \
        else col.type
    assert back.type == want_type
    assert back.null_count == 2
    assert back.to_pylist() == col.cast(want_type).to_pylist()


def test_key_words_without_nulls_gives_no_mask():
    kw = _key_words()(["a", "s"], null_keys=True)
    t = pa.table({"a": pa.array([3, 4], type=pa.int64()),
                  "s": pa.array(["u", "v"])})
    words, masks = kw.words(t, _NoDeviceOps)
    assert masks == [None, None]
    assert words[0].tolist() == [3, 4]
    assert kw.to_arrow("a", kw.decode("a", words[0])).to_pylist() == [3, 4]


def test_key_words_zero_under_null_whatever_the_buffer_held():
    """Arrow promises nothing about the slot under a null: hand-built
    arrays whose value buffers hold junk there."""
    junk = np.array([11, C.I64_MIN, 22, -1, 33], dtype=np.int64)
    valid = np.packbits(np.array([1, 0, 1, 0, 1], dtype=bool),
                        bitorder="little")
    col = pa.Array.from_buffers(pa.int64(), 5,
                                [pa.py_buffer(valid), pa.py_buffer(junk)])
    assert col.to_pylist() == [11, None, 22, None, 33]
    kw = _key_words()(["k"], null_keys=True)
    words, masks = kw.words(pa.table({"k": col}), _NoDeviceOps)
    assert words[0].tolist() == [11, 0, 22, 0, 33]
    assert masks[0].tolist() == [True, False, True, False, True]


def test_key_words_mask_of_a_sliced_array():
    """A slice whose offset is no multiple of 8: the mask is that of the
    slice's own rows."""
    n = 40
    full_mask = (np.arange(n) % 3) != 0
    col = pa.array(np.arange(n, dtype=np.int64), mask=~full_mask)
    s = pa.array(["s%d" % i if ok else None
                  for i, ok in enumerate(full_mask)])
    t = pa.table({"k": col, "s": s}).slice(5, 21)
    kw = _key_words()(["k", "s"], null_keys=True)
    words, masks = kw.words(t, _NoDeviceOps)
    want = full_mask[5:26]
    for m in masks:
        assert np.array_equal(m, want)
    assert np.array_equal(words[0], np.where(want, np.arange(5, 26), 0))
    assert kw.to_arrow("s", kw.decode("s", words[1], masks[1]),
                       masks[1]).to_pylist() == t.column("s").to_pylist()


def test_default_key_words_still_refuse_nulls():
    kw = _key_words()(["k"])
    with pytest.raises(TypeError, match="null keys are not supported"):
        kw.check(pa.table({"k": pa.array([1, None])}), "test")
    # and words() keeps its one return value
    out = kw.words(pa.table({"k": pa.array([1, 2])}), _NoDeviceOps)
    assert isinstance(out, list) and out[0].tolist() == [1, 2]


def test_null_keys_without_device_keys_raises():
    from quokka_amd.executors import GPUAggExecutor
    with pytest.raises(ValueError, match="device_keys"):
        GPUAggExecutor(["g"], None, "sum(x) as sx", null_keys=True)
    GPUAggExecutor(["g"], None, "sum(x) as sx", device_keys=True,
                   null_keys=True)


def test_order_by_puts_null_keys_last_both_ways():
    """The host order-by of the null_keys path against pyarrow's sort_by,
    whose default places nulls at the end in either direction."""
    from quokka_amd.executors import GPUAggExecutor
    vals = np.array([3, 0, 1, 0, 2], dtype=np.int64)
    mask = np.array([1, 0, 1, 0, 1], dtype=bool)
    tie = np.array([0, 1, 2, 0, 4], dtype=np.int64)
    t = pa.table({"g": pa.array(vals, mask=~mask), "h": tie})
    for d, ad in (("asc", "ascending"), ("desc", "descending")):
        ex = GPUAggExecutor(["g", "h"], [("g", d), ("h", "asc")],
                            "sum(x) as sx", device_keys=True, null_keys=True)
        order = ex._order_by({"g": vals, "h": tie}, {"g": mask})
        want = t.sort_by([("g", ad), ("h", "ascending")])
        assert t.take(pa.array(order)).equals(want), d


def test_broadcast_join_passes_null_keys_on():
    from quokka_amd import GPUBroadcastJoinExecutor
    small = pa.table({"k": pa.array([1, None, 3], type=pa.int64()),
                      "v": [1.0, 2.0, 3.0]})
    ex = GPUBroadcastJoinExecutor(small, on="k", null_keys=True)
    assert ex.null_keys
    assert ex._small_host["k"].dtype == np.int64, "no float64 detour"
    assert ex._small_host["k"].tolist() == [1, 0, 3]
    assert ex._small_key_mask.tolist() == [True, False, True]
    assert not GPUBroadcastJoinExecutor(small, on="k").null_keys
