"""Null keys: a pure-numpy model of qk_key_null_words and
qk_nullword_to_valid (DESIGN.md §3a'''), of the codes a nullable key
dictionary hands out, and of the join rules (a NULL key matches nothing),
plus the named case lists the CPU and GPU tests share. The CPU tests hold
the model against pyarrow Acero; the GPU tests hold the kernels against the
model."""
import numpy as np

I64_MIN = np.iinfo(np.int64).min

# what a caller's column may hold under a null: the former sentinel, -1,
# and a value that also occurs as a valid key (KEY_LO..KEY_HI below)
JUNK = np.array([I64_MIN, -1, 2], dtype=np.int64)
KEY_LO, KEY_HI = -3, 4


def valid_nbytes(n):
    return ((int(n) + 63) // 64) * 8 + 8


def pack_valid(mask):
    """bool mask -> bitmap bytes, bits past the end 0, whole words + 8."""
    out = np.zeros(valid_nbytes(len(mask)), dtype=np.uint8)
    bits = np.packbits(np.asarray(mask, dtype=bool), bitorder="little")
    out[:len(bits)] = bits
    return out


def null_words(cols, masks):
    """Model of qk_key_null_words. cols: K int64 arrays; masks: K bool
    arrays (True = valid) or None. -> (canon: K arrays or None where the
    key has no bitmap, nullw: W int64 arrays)."""
    k_n = len(cols)
    n = len(cols[0])
    canon = [None if m is None else np.where(m, c, 0).astype(np.int64)
             for c, m in zip(cols, masks)]
    nullw = np.zeros(((k_n + 63) // 64, n), dtype=np.uint64)
    for k, m in enumerate(masks):
        if m is not None:
            nullw[k // 64] |= (~m).astype(np.uint64) << np.uint64(k % 64)
    return canon, [w.view(np.int64) for w in nullw]


def nullword_to_valid(null_col, bit, g):
    """Model of qk_nullword_to_valid -> (bitmap bytes of valid_nbytes(g),
    null count)."""
    w = np.asarray(null_col[:g]).view(np.uint64)
    valid = ((w >> np.uint64(bit)) & np.uint64(1)) == 0
    return pack_valid(valid), int(g - valid.sum())


def key_rows(cols, masks):
    """The K + W words of every row as an (n, K + W) int64 array: two rows
    are one key exactly when their rows here are equal."""
    canon, nullw = null_words(cols, masks)
    words = [c if k is None else k for c, k in zip(cols, canon)]
    return np.stack(words + nullw, axis=1)


def first_seen_codes(rows, seen=None):
    """Dense ids in order of first occurrence over the (n, words) array,
    continuing `seen` (dict tuple -> id) from earlier batches."""
    seen = {} if seen is None else seen
    out = np.empty(len(rows), dtype=np.int64)
    for i, r in enumerate(map(tuple, rows.tolist())):
        out[i] = seen.setdefault(r, len(seen))
    return out, seen


def same_partition(a, b):
    """True when code arrays a and b put the rows into the same groups."""
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


def join(build_keys, build_valid, probe_keys, probe_valid, mode):
    """Model of JoinTable with validity. mode 0 -> sorted (probe row,
    build row) pairs; 1 / 2 -> sorted probe rows with / without a match.
    A null key matches nothing on either side; the value under it is never
    looked at."""
    by_key = {}
    for b, (k, ok) in enumerate(zip(build_keys.tolist(),
                                    build_valid.tolist())):
        if ok:
            by_key.setdefault(k, []).append(b)
    pairs, hit, miss = [], [], []
    for p, (k, ok) in enumerate(zip(probe_keys.tolist(),
                                    probe_valid.tolist())):
        rows = by_key.get(k, []) if ok else []
        (hit if rows else miss).append(p)
        pairs += [(p, b) for b in rows]
    return sorted(pairs) if mode == 0 else (hit if mode == 1 else miss)


# ---- qk_key_null_words cases: every n against every K -------------------
NULL_WORD_N = [0, 1, 63, 64, 65, 129, 4097]
NULL_WORD_K = [1, 3, 64, 65]
# column k is of kind k % 4
KINDS = ("random nulls", "no bitmap", "all null", "all valid")


def null_word_case(n, k_n, seed=0):
    """-> (cols, masks): key values in [KEY_LO, KEY_HI), the slots under a
    null overwritten with JUNK in turn; a "random nulls" column is null at
    rows 0, 63, 64 and n - 1 wherever those exist."""
    rng = np.random.default_rng(1000 * k_n + n + seed)
    cols, masks = [], []
    for k in range(k_n):
        c = rng.integers(KEY_LO, KEY_HI, n).astype(np.int64)
        kind = KINDS[k % 4]
        if kind == "no bitmap":
            m = None
        elif kind == "all null":
            m = np.zeros(n, dtype=bool)
        elif kind == "all valid":
            m = np.ones(n, dtype=bool)
        else:
            m = rng.random(n) > 0.3
            for r in (0, 63, 64, n - 1):
                if 0 <= r < n:
                    m[r] = False
        if m is not None:
            c[~m] = JUNK[np.arange(n)[~m] % len(JUNK)]
        cols.append(c)
        masks.append(m)
    return cols, masks


NULLWORD_TO_VALID_G = [0, 1, 63, 64, 65, 1000]


# ---- group / distinct cases: small K, held against Acero on the CPU -----
def _tuples_case():
    # (NULL, 0), (0, NULL), (0, 0), (NULL, NULL), each twice, junk below
    a = np.array([7, 0, 0, -1, I64_MIN, 0, 0, 2], dtype=np.int64)
    b = np.array([0, 7, 0, I64_MIN, 0, -1, 0, 2], dtype=np.int64)
    ma = np.array([0, 1, 1, 0, 0, 1, 1, 0], dtype=bool)
    mb = np.array([1, 0, 1, 0, 1, 0, 1, 0], dtype=bool)
    return [a, b], [ma, mb]


GROUP_CASES = {
    "four_tuples": _tuples_case(),
    "one_key_129": null_word_case(129, 1),
    "three_keys_4097": null_word_case(4097, 3),
    "four_keys_65": null_word_case(65, 4),
}


# ---- join cases ----------------------------------------------------------
JOIN_N_PROBE = [1, 64, 65, 1000]


def join_case(n_probe, seed=0):
    """Two build batches and one probe batch, (keys, mask) each. Build
    keys repeat; null build rows hold INT64_MIN or a key the probe side
    holds; null probe rows hold a built key."""
    rng = np.random.default_rng(77 + n_probe + seed)
    builds = []
    for nb in (40, 25):
        k = rng.integers(0, 20, nb).astype(np.int64) * 3
        m = rng.random(nb) > 0.25
        m[0] = False
        nulls = np.nonzero(~m)[0]
        k[nulls[0::2]] = I64_MIN
        k[nulls[1::2]] = 3 * (nulls[1::2] % 20)    # a key probes will ask for
        builds.append((k, m))
    pk = rng.integers(0, 30, n_probe).astype(np.int64) * 3
    pm = rng.random(n_probe) > 0.2
    pm[-1] = False
    built = np.concatenate([k[m] for k, m in builds])
    pk[~pm] = built[np.arange(int((~pm).sum())) % len(built)]
    return builds, (pk, pm)
