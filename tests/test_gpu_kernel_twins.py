"""Edges of the kernels that share one body (ordered compaction
and nullable twins): the ordered compaction behind the filter, the Q3
extract and the newline index where a block takes more than one 256-row
step (n > MAX_BLOCKS * BLOCK = 524,288), and the *_valid entry points of
join and dense accumulate against their plain twins. Everything is checked
exactly against numpy; hash tables stay at or below half load."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

I64_MIN = np.iinfo(np.int64).min


@pytest.fixture(scope="module")
def gpu():
    from quokka_amd import shim
    shim.init(0)
    return shim


def _zeroed(shim, dtype, n):
    return shim.DevColumn.from_numpy(np.zeros(n, dtype=dtype))


# ---- 1. filter edges ---------------------------------------------------------
FILTER_N = [1, 63, 64, 65, 255, 256, 257, 524288, 524289, 600001]
TWO_STEP_N = FILTER_N[-2:]      # 512-row chunks: two steps per block


def _filter_masks(n):
    rng = np.random.default_rng(n)
    i = np.arange(n)
    masks = {
        "all": np.ones(n, dtype=bool),
        "none": np.zeros(n, dtype=bool),
        "half": rng.random(n) < 0.5,
        "last": i == n - 1,
        "lane0": i % 64 == 0,
    }
    if n in TWO_STEP_N:
        masks["second_step"] = i % 512 >= 256
    return masks


@pytest.mark.parametrize("dtype", [np.int32, np.uint8, np.float64])
@pytest.mark.parametrize("n", FILTER_N)
def test_filter_ordered_at_step_edges(gpu, n, dtype):
    from quokka_amd import ops, shim
    for name, mask in _filter_masks(n).items():
        col = shim.DevColumn.from_numpy(mask.astype(dtype))
        idx, cnt = ops.filter_col(col, ops.GT, 0)
        got = idx.to_numpy(cnt)
        col.free()
        idx.free()
        assert cnt == int(mask.sum()), name
        assert np.array_equal(got, np.nonzero(mask)[0]), name


# ---- 2. Q3 extract, direct ---------------------------------------------------
GUARD_I64, GUARD_I32, GUARD_F64 = -0x5A5A5A5A5A5A5A5A, -0x5A5A5A5A, -12345.5


def _q3_extract(shim, keys, head, sums, out_cap):
    """One qk_q3_extract call into buffers of out_cap + 1 words whose last
    word is a guard -> (count, keys, rows, sums, guards intact)."""
    dk, dh, ds = (shim.DevColumn.from_numpy(a) for a in (keys, head, sums))
    ok = shim.DevColumn.from_numpy(np.full(out_cap + 1, GUARD_I64, np.int64))
    orow = shim.DevColumn.from_numpy(np.full(out_cap + 1, GUARD_I32, np.int32))
    osum = shim.DevColumn.from_numpy(np.full(out_cap + 1, GUARD_F64))
    cur = _zeroed(shim, np.uint64, 1)
    shim.call("qk_q3_extract", None, dk.ptr, dh.ptr, ds.ptr,
              shim.c_u64(len(keys)), ok.ptr, orow.ptr, osum.ptr,
              shim.c_u64(out_cap), cur.ptr)
    shim.call("qk_stream_sync", None)
    cnt = int(cur.to_numpy()[0])
    k, r, s = ok.to_numpy(), orow.to_numpy(), osum.to_numpy()
    for d in (dk, dh, ds, ok, orow, osum, cur):
        d.free()
    intact = k[out_cap] == GUARD_I64 and r[out_cap] == GUARD_I32 and \
        s[out_cap] == GUARD_F64
    return cnt, k[:out_cap], r[:out_cap], s[:out_cap], intact


@pytest.mark.parametrize("cap", [16, 1 << 20])
def test_q3_extract_direct(gpu, cap):
    rng = np.random.default_rng(cap)
    kind = rng.integers(0, 3, cap)      # 0 empty, 1 live zero sum, 2 live
    kind[:3] = [2, 0, 1]
    kind[-1] = 2                        # the last slot of the last step
    keys = np.where(kind == 0, I64_MIN,
                    rng.integers(1, 1 << 40, cap)).astype(np.int64)
    head = rng.integers(0, 1 << 30, cap).astype(np.int32)
    sums = np.where(kind == 2, rng.integers(1, 1000, cap), 0).astype(
        np.float64)
    sums[kind == 0] = 7.0               # a sum under an empty slot is not live
    live = np.nonzero(kind == 2)[0]
    cnt, k, r, s, intact = _q3_extract(gpu, keys, head, sums, len(live))
    assert cnt == len(live) and intact
    assert np.array_equal(k, keys[live])
    assert np.array_equal(r, head[live])
    assert np.array_equal(s, sums[live])
    # one output row short: counted in full, nothing written past out_cap
    short = len(live) - 1
    cnt, k, r, s, intact = _q3_extract(gpu, keys, head, sums, short)
    assert cnt == len(live), "the full count"
    assert intact, "guard word after out_cap"
    assert np.array_equal(k, keys[live][:short])
    assert np.array_equal(r, head[live][:short])
    assert np.array_equal(s, sums[live][:short])


# ---- 3. newline index, direct ------------------------------------------------
def _newlines(shim, b, n, data_start):
    db = shim.DevColumn.from_numpy(b)
    out = _zeroed(shim, np.uint64, max(1, n))
    cnt = _zeroed(shim, np.uint64, 1)
    shim.call("qk_csv_newlines", None, shim.c_u64(data_start), shim.c_u64(n),
              db.ptr, out.ptr, cnt.ptr)
    shim.call("qk_stream_sync", None)
    k = int(cnt.to_numpy()[0])
    pos = out.to_numpy()[:k]
    for d in (db, out, cnt):
        d.free()
    return k, pos


@pytest.mark.parametrize("n", [600001, 8, 7])
def test_csv_newlines_direct(gpu, n):
    rng = np.random.default_rng(n)
    b = rng.choice(np.array([10, 44, 48, 49, 34], dtype=np.uint8), 600001)
    b[6] = 10                           # in front of data_start: not indexed
    b[7] = 10
    b[n - 1] = 10                       # the last byte
    want = np.nonzero(b[:n] == 10)[0]
    want = want[want >= 7].astype(np.uint64)
    k, pos = _newlines(gpu, b, n, 7)
    assert k == len(want)
    assert np.array_equal(pos, want)
    if n == 7:
        assert k == 0, "empty span: the caller-zeroed count stays 0"


# ---- 4. twin equivalence -----------------------------------------------------
def _pow2_at_least(n):
    c = 16
    while c < n:
        c <<= 1
    return c


def _numpy_join(bk, pk, mode):
    order = np.argsort(bk, kind="stable")
    lo = np.searchsorted(bk[order], pk, "left")
    hi = np.searchsorted(bk[order], pk, "right")
    if mode == 1:
        return sorted(np.nonzero(hi > lo)[0].tolist())
    if mode == 2:
        return sorted(np.nonzero(hi == lo)[0].tolist())
    return sorted((int(p), int(order[j])) for p in range(len(pk))
                  for j in range(lo[p], hi[p]))


def _join(shim, bk, pk, mode, valid, out_cap):
    """Raw build + probe; with `valid` the *_valid entry points and an
    all-ones bitmap. -> sorted probe rows (semi/anti) or pairs (inner)."""
    cap = _pow2_at_least(2 * len(bk))
    slot_keys = shim.DevColumn.from_numpy(np.full(cap, I64_MIN, np.int64))
    slot_head = shim.DevColumn.from_numpy(np.full(cap, -1, np.int32))
    chain = shim.DevColumn.from_numpy(np.full(len(bk), -1, np.int32))
    dbk, dpk = shim.DevColumn.from_numpy(bk), shim.DevColumn.from_numpy(pk)
    bits = lambda n: shim.DevColumn.from_numpy(           # noqa: E731
        np.full((n + 63) // 64, ~np.uint64(0), dtype=np.uint64))
    bvalid, pvalid = (bits(len(bk)), bits(len(pk))) if valid else (None, None)
    out_p = _zeroed(shim, np.uint32, max(1, out_cap))
    out_b = _zeroed(shim, np.uint32, max(1, out_cap))
    cur = _zeroed(shim, np.uint64, 1)
    table = (slot_keys.ptr, slot_head.ptr, chain.ptr, shim.c_u64(cap))
    outs = (mode, out_p.ptr, out_b.ptr if mode == 0 else None,
            shim.c_u64(out_cap), cur.ptr)
    if valid:
        shim.call("qk_join_build_valid", None, shim.c_u64(len(bk)), dbk.ptr,
                  bvalid.ptr, shim.c_u32(0), *table)
        shim.call("qk_join_probe_valid", None, shim.c_u64(len(pk)), dpk.ptr,
                  pvalid.ptr, *table, *outs)
    else:
        shim.call("qk_join_build", None, shim.c_u64(len(bk)), dbk.ptr,
                  shim.c_u32(0), *table)
        shim.call("qk_join_probe", None, shim.c_u64(len(pk)), dpk.ptr,
                  *table, *outs)
    shim.call("qk_stream_sync", None)
    cnt = int(cur.to_numpy()[0])
    assert cnt <= out_cap
    p, b = out_p.to_numpy()[:cnt].tolist(), out_b.to_numpy()[:cnt].tolist()
    for d in (slot_keys, slot_head, chain, dbk, dpk, out_p, out_b, cur):
        d.free()
    if valid:
        bvalid.free()
        pvalid.free()
    return sorted(zip(p, b)) if mode == 0 else sorted(p)


@pytest.mark.parametrize("n", [1, 65, 257, 70001])
def test_join_valid_all_ones_equals_plain(gpu, n):
    rng = np.random.default_rng(n)
    bk = rng.integers(0, max(1, n // 2), n).astype(np.int64)  # duplicates
    pk = rng.integers(0, n, n).astype(np.int64)               # ~half miss
    if n > 1:
        assert len(np.unique(bk)) < n
    for mode in (0, 1, 2):
        want = _numpy_join(bk, pk, mode)
        plain = _join(gpu, bk, pk, mode, False, len(want))
        twin = _join(gpu, bk, pk, mode, True, len(want))
        assert plain == want, mode
        assert twin == want, mode


def test_dense_acc_valid_without_bitmaps_equals_plain(gpu):
    shim = gpu
    rng = np.random.default_rng(11)
    n, ncodes, ops = 70001, 300, [0, 1, 2]      # SUM, MIN, MAX
    nvals, rstride = 3, 4
    used = rng.choice(ncodes, 200, replace=False)
    codes = used[rng.integers(0, len(used), n)].astype(np.uint32)
    vals = [rng.integers(-50, 51, n).astype(np.float64) for _ in ops]
    init = np.array([0.0, np.inf, -np.inf])
    want = np.zeros((ncodes, rstride))
    want[:, :nvals] = init
    np.add.at(want[:, 0], codes, vals[0])
    np.minimum.at(want[:, 1], codes, vals[1])
    np.maximum.at(want[:, 2], codes, vals[2])

    dcodes = shim.DevColumn.from_numpy(codes)
    dvals = [shim.DevColumn.from_numpy(v) for v in vals]
    vptrs = shim.DevColumn.from_numpy(
        np.array([d.ptr.value for d in dvals], dtype=np.uint64))
    bptrs = _zeroed(shim, np.uint64, nvals)     # every valid[c] is 0
    inits = shim.DevColumn.from_numpy(init)
    dops = shim.DevColumn.from_numpy(np.array(ops, dtype=np.int32))
    err = _zeroed(shim, np.uint32, 1)
    seen = _zeroed(shim, np.uint64, ncodes)
    recs = []
    for twin in (False, True):
        acc = shim.DevColumn(np.float64, ncodes * rstride)
        shim.call("qk_groupby_dense_init", None, acc.ptr, shim.c_u64(0),
                  shim.c_u64(ncodes), rstride, nvals, inits.ptr)
        head = (None, shim.c_u64(n), dcodes.ptr, shim.c_u32(ncodes),
                vptrs.ptr)
        tail = (dops.ptr, nvals, rstride, acc.ptr)
        if twin:
            shim.call("qk_groupby_dense_acc_valid", *head, bptrs.ptr, *tail,
                      seen.ptr, err.ptr)
        else:
            shim.call("qk_groupby_dense_acc", *head, *tail, err.ptr)
        shim.call("qk_stream_sync", None)
        recs.append(acc.to_numpy().reshape(ncodes, rstride))
        acc.free()
    assert int(err.to_numpy()[0]) == 0
    assert recs[0].tobytes() == want.tobytes(), "plain against numpy"
    assert recs[1].tobytes() == recs[0].tobytes(), "bit-identical records"
    want_seen = np.zeros(ncodes, dtype=np.uint64)
    want_seen[np.unique(codes)] = (1 << nvals) - 1
    assert np.array_equal(seen.to_numpy(), want_seen)
    for d in [dcodes, vptrs, bptrs, inits, dops, err, seen] + dvals:
        d.free()
