"""Host half of the wide-key group-by (GPUAggExecutor(device_keys=True),
GPUDistinctExecutor over a key list): constructor and pickle contract,
the key-column -> 64-bit-word conversion with its inverse, and the
refusal of null keys. No GPU."""
import pickle

import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")

I64 = np.iinfo(np.int64)


def test_constructor_accepts_device_keys_and_pickles():
    from quokka_amd import GPUAggExecutor
    keys = ["k%d" % i for i in range(7)]
    a = GPUAggExecutor(keys, [("k0", "asc")], "sum(x) as sx, min(y) as mn",
                       device_keys=True)
    assert a.device_keys is True
    b = pickle.loads(pickle.dumps(a))
    assert b.device_keys is True and b.groupby_keys == keys
    assert b.sum_cols == ["x", "y"] and b.agg_ops == [0, 1]
    # the default stays the composite path
    assert GPUAggExecutor(["g"], None, "sum(x) as sx").device_keys is False


def test_distinct_constructor_key_lists():
    from quokka_amd.executors import GPUDistinctExecutor
    d = GPUDistinctExecutor(["a", "b"])
    assert d.keys == ["a", "b"]
    pickle.loads(pickle.dumps(d))
    assert GPUDistinctExecutor("a").keys == "a"
    assert GPUDistinctExecutor(["a"]).keys == "a"
    with pytest.raises(TypeError):
        GPUDistinctExecutor(["a", 3])


@pytest.mark.parametrize("dtype", [np.int8, np.int16, np.int32, np.int64,
                                   np.uint8, np.uint16, np.uint32,
                                   np.uint64, np.bool_])
def test_integer_words_round_trip(dtype):
    from quokka_amd.executors import key_to_words, words_to_key
    if dtype is np.bool_:
        arr = np.array([True, False, True])
    else:
        info = np.iinfo(dtype)
        arr = np.array([info.min, info.max, 0, 1, info.max - 1], dtype=dtype)
    w = key_to_words(arr)
    assert w.dtype == np.int64 and len(w) == len(arr)
    back = words_to_key(w, arr.dtype)
    assert back.dtype == arr.dtype
    assert np.array_equal(back, arr)
    # distinct values keep distinct words
    assert len(np.unique(w)) == len(np.unique(arr))
    if np.dtype(dtype).kind == "i":
        assert np.array_equal(w, arr.astype(np.int64))      # widened by value


def test_date_words_round_trip():
    from quokka_amd.executors import key_to_words, words_to_key
    d = np.array(["1992-01-01", "1998-08-02", "1969-12-31"],
                 dtype="datetime64[D]")
    w = key_to_words(d)
    assert w.tolist() == [8035, 10440, -1]
    assert np.array_equal(words_to_key(w, d.dtype), d)
    ms = d.astype("datetime64[ms]")
    wm = key_to_words(ms)
    assert wm.tolist() == [8035 * 86400000, 10440 * 86400000, -86400000]
    assert np.array_equal(words_to_key(wm, ms.dtype), ms)


def test_float_words_normalise_zero_and_nan():
    from quokka_amd.executors import key_to_words, words_to_key
    nan_a = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]
    nan_b = np.array([0xFFF0000000000123], dtype=np.uint64).view(np.float64)[0]
    assert np.isnan(nan_a) and np.isnan(nan_b)
    arr = np.array([0.0, -0.0, nan_a, nan_b, 1.5, -1.5, np.inf, -np.inf,
                    5e-324])
    before = arr.copy()
    w = key_to_words(arr)
    assert np.array_equal(arr.view(np.int64), before.view(np.int64)), \
        "input must not be modified"
    assert w[0] == w[1] == 0                       # -0.0 groups with +0.0
    assert w[2] == w[3] == 0x7FF8000000000000      # one canonical NaN
    assert len(set(w[4:].tolist())) == 5
    back = words_to_key(w, np.float64)
    assert not np.signbit(back[1])
    assert np.isnan(back[2]) and np.isnan(back[3])
    assert np.array_equal(back[4:], arr[4:])


def test_float32_column_round_trips():
    from quokka_amd.executors import key_to_words, words_to_key
    rng = np.random.default_rng(5)
    arr = rng.standard_normal(1000).astype(np.float32)
    arr[:3] = [np.float32(1e-45), np.float32(3.4028235e38), np.float32(-0.0)]
    w = key_to_words(arr)
    assert w.dtype == np.int64
    # the word is the float64 bit pattern of the widened value
    assert w[3] == np.float64(arr[3]).view(np.int64)
    back = words_to_key(w, np.float32)
    assert back.dtype == np.float32
    assert np.array_equal(back[:2], arr[:2]) and np.array_equal(back[3:],
                                                                arr[3:])
    assert back[2] == 0 and not np.signbit(back[2])


def test_unsupported_key_dtype_raises():
    from quokka_amd.executors import key_to_words
    with pytest.raises(TypeError):
        key_to_words(np.array(["a", "b"], dtype=object))


def test_arrow_key_types_to_words_and_back():
    """The Arrow layer of the conversion, on the host: date32 / date64 /
    timestamp / bool / float32 columns become words and decode back to
    their original Arrow type."""
    import datetime as dt
    from quokka_amd.executors import _KeyWords
    t = pa.table({
        "d32": pa.array([dt.date(1995, 3, 15), dt.date(1969, 1, 1)],
                        type=pa.date32()),
        "d64": pa.array([dt.date(1995, 3, 15), dt.date(1969, 1, 1)],
                        type=pa.date64()),
        "ts": pa.array([1, -5], type=pa.timestamp("us")),
        "b": pa.array([True, False]),
        "f32": pa.array([1.25, -0.0], type=pa.float32()),
        "i16": pa.array([-7, 9], type=pa.int16()),
    })
    kw = _KeyWords(t.column_names)
    kw.check(t, "test")
    words = kw.words(t, ops=None)          # no string key: no device use
    assert all(w.dtype == np.int64 for w in words)
    assert words[0].tolist() == [9204, -365]
    for name, w in zip(t.column_names, words):
        back = kw.to_arrow(name, kw.decode(name, w))
        assert back.type == t.schema.field(name).type
        want = t.column(name).combine_chunks()
        if name == "f32":
            assert back.to_pylist() == [1.25, 0.0]
        else:
            assert back.equals(want), name


def test_nullable_key_column_raises_typeerror():
    from quokka_amd import GPUAggExecutor
    from quokka_amd.executors import GPUDistinctExecutor
    t = pa.table({"a": pa.array([1, None, 3], type=pa.int64()),
                  "b": pa.array([1, 2, 3], type=pa.int64()),
                  "v": pa.array([1.0, 2.0, 3.0])})
    ex = GPUAggExecutor(["b", "a"], None, "sum(v) as s", device_keys=True)
    with pytest.raises(TypeError, match="null"):
        ex.execute([t], 0, 0)
    with pytest.raises(TypeError, match="null"):
        GPUDistinctExecutor(["a", "b"]).execute([t], 0, 0)
