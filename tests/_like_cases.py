"""Shared LIKE test material: the `re` oracle, the seeded fuzz generator
and Arrow-layout helpers. Host-only and deterministic;
tests/test_like_cpu.py runs the matcher on the CPU against it and
tests/test_gpu_like.py the kernels."""
import re

import numpy as np

FUZZ_SEED = 20240607
PAT_ALPHABET = "ab%_"
STR_ALPHABET = "abé"


def like_regex(pattern, exact=False):
    """SQL LIKE pattern -> compiled regex: % -> .*, _ -> ., the rest
    escaped, re.S, used with fullmatch (the translation jit.py uses for
    dictionary-coded columns)."""
    if exact:
        return re.compile(re.escape(pattern), re.S)
    return re.compile("".join(".*" if ch == "%" else "." if ch == "_"
                              else re.escape(ch) for ch in pattern), re.S)


def oracle(pattern, strings, negate=False, exact=False):
    """-> np.uint8 flags, Python `re` on the decoded strings."""
    rx = like_regex(pattern, exact)
    m = np.fromiter((rx.fullmatch(s) is not None for s in strings),
                    dtype=bool, count=len(strings))
    return (m ^ bool(negate)).astype(np.uint8)


def fuzz_cases(npat, nstr, seed=FUZZ_SEED):
    """-> (patterns, strings): patterns of length 0-8 over {a, b, %, _},
    strings of length 0-12 over {a, b, é}."""
    rng = np.random.default_rng(seed)
    pats = ["".join(PAT_ALPHABET[i] for i in
                    rng.integers(0, len(PAT_ALPHABET), rng.integers(0, 9)))
            for _ in range(npat)]
    strs = ["".join(STR_ALPHABET[i] for i in
                    rng.integers(0, len(STR_ALPHABET), rng.integers(0, 13)))
            for _ in range(nstr)]
    return pats, strs


def arrow_layout(strings, offset_dtype=np.int64):
    """list of str -> (offsets[n+1], bytes np.uint8) in Arrow layout."""
    enc = [s.encode() for s in strings]
    off = np.zeros(len(enc) + 1, dtype=offset_dtype)
    if enc:
        np.cumsum([len(b) for b in enc], out=off[1:])
    data = np.frombuffer(b"".join(enc), dtype=np.uint8)
    return off, data


WORDS = ("furiously quickly carefully slyly blithely final regular express "
         "pending ironic bold even silent deposits accounts packages "
         "theodolites instructions foxes pinto beans platelets ideas "
         "forest green BRASS special requests Customer Complaints").split()


def comments(rng, n, lo=0, hi=40, plant=None, frac=0.02):
    """n word-salad strings of lo..hi bytes; `plant` = (w1, w2) puts
    'w1 ... w2' into about `frac` of the rows."""
    out = []
    for _ in range(n):
        target = int(rng.integers(lo, hi + 1))
        s = ""
        while len(s) < target:
            s += WORDS[int(rng.integers(0, len(WORDS)))] + " "
        out.append(s[:target])
    if plant:
        for i in np.nonzero(rng.random(n) < frac)[0]:
            out[i] = "%s %s %s %s" % (out[i][:8], plant[0],
                                      WORDS[int(rng.integers(0, 8))],
                                      plant[1])
    return out
