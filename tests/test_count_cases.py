"""CPU: the inputs of tests/count_cases.py reach what they claim, by the references alone.

The restated hash equals the library's own (bpe_short_hash_host calls stage.h's short_hash) on
100 000 random words of every length 2..16, and the restated constants equal the constexpr lines of
csrc/count.hip, csrc/count.h and csrc/stage.h, so a retune fails here and not in the premise of the
GPU tests.  For every case the oracle's word table equals the planned multiset; then, per family,
the condition the case is built for, computed from the text and the restated hash.
"""
from __future__ import annotations

import ctypes
import functools
import pathlib
import re

import numpy as np
import pytest

import count_cases as C
from oracle import oracle

bpe_amd = pytest.importorskip("bpe_amd")
from bpe_amd import _lib  # noqa: E402

CSRC = pathlib.Path(__file__).resolve().parent.parent / "transformer-lm_amd" / "csrc"


# ---------------------------------------------------------------------- the hash and the constants
def library_hash(words: np.ndarray) -> np.ndarray:
    fn = _lib.lib().bpe_short_hash_host
    fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
    fn.restype = ctypes.c_int
    words = np.ascontiguousarray(words)
    out = np.zeros(len(words), dtype=np.uint64)
    assert fn(words.ctypes.data, len(words), words.shape[1], out.ctypes.data) == 0
    return out


@pytest.mark.parametrize("length", range(2, 17))
def test_restated_hash_equals_the_library(length):
    rng = np.random.default_rng(1000 + length)
    words = rng.integers(0, 256, (100_000, length), dtype=np.uint8)
    words[:1000, rng.integers(0, length, 1000)] = 0          # NUL bytes, trailing ones among them
    words[0] = 0
    words[1] = 255
    got, want = C.hash_rows(words), library_hash(words)
    assert np.array_equal(got, want)
    assert C.hash_word(bytes(words[7])) == int(want[7])


def test_library_hash_refuses_other_lengths():
    fn = _lib.lib().bpe_short_hash_host
    fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
    buf, out = np.zeros(64, dtype=np.uint8), np.zeros(4, dtype=np.uint64)
    for length in (0, 1, 17):
        assert fn(buf.ctypes.data, 1, length, out.ctypes.data) == _lib.BPE_E_ARG
    assert "bpe_short_hash_host" not in (CSRC.parent.parent / "include" / "bpe355.h").read_text()


def _source_constants():
    """every `constexpr <type> kName = <expression>;` of the three files, evaluated in order"""
    env: dict = {}
    for name in ("stage.h", "count.h", "count.hip"):
        for m in re.finditer(r"^\s*constexpr\s+(?:unsigned\s+long\s+long|unsigned|int|size_t)\s+(k\w+)\s*=\s*([^;]+);",
                             (CSRC / name).read_text(), flags=re.M):
            expr = re.sub(r"(?<=\d)(?:ULL|ull|u|U)\b", "", m.group(2)).replace("/", "//")
            try:
                env[m.group(1)] = eval(expr, {"__builtins__": {}}, dict(env))   # noqa: S307 (the project's own source)
            except Exception:   # an expression this test has no use for
                continue
    return env


def test_restated_constants_equal_the_source():
    env = _source_constants()
    for mine, (_file, theirs) in C.SOURCE_CONSTANTS.items():
        assert theirs in env, theirs
        assert getattr(C, mine) == env[theirs], (mine, theirs)
    assert C.K_REC_RESERVE == 9217
    text = (CSRC / "count.hip").read_text()
    # the shifts the case module restates, as the kernels write them
    assert "(unsigned)(h >> 40) & (kCache2 - 2)" in text
    assert "(unsigned)(h >> 20) & (kRedSlots - 1)" in text
    assert "h >> (64 - kCoarseBits)" in text and "(h >> (64 - kBinBits))" in text
    assert "c < (1ULL << kCntBits)" in text and "(c << 45)" in text and 45 + C.K_CNT_BITS == 64
    assert "(unsigned)(h >> 24) & (kLongSlots - 1)" in text


# ---------------------------------------------------------------------- every case
@functools.lru_cache(maxsize=None)
def _oracle_words(name):
    return oracle.word_counts(C.CASES[name]().data)


@functools.lru_cache(maxsize=None)
def _pretokens(name):
    """(starts, lengths) of the text's pre-tokens, by the oracle's scanner"""
    p = np.array(oracle.pretokenize(C.CASES[name]().data), dtype=np.uint64)
    return p[:, 0], p[:, 1]


@pytest.mark.parametrize("name", list(C.CASES))
def test_oracle_equals_the_plan(name):
    c = C.CASES[name]()
    assert _oracle_words(name) == c.plan
    assert len(c.data) <= 12 << 20
    assert all(k in ("BPE355_STREAM_WG", "BPE355_LONG_SEG") for k in c.knobs)


def test_candidates():
    cand = C.candidates()
    assert 0 < cand.coarse < C.K_COARSE - 1 and cand.fine >> C.K_COARSE_BITS == cand.coarse
    assert np.all(C.coarse_bin(cand.coarse_h) == np.uint64(cand.coarse))
    assert len(np.unique(cand.coarse_lo)) == len(cand.coarse_lo) >= max(C.COARSE_SIZES.values())
    assert cand.fullest >= C.N_FINE
    assert np.array_equal(C.short_hash(cand.other_lo, 0, 8), cand.other_h)
    words = np.frombuffer(C.text_of(cand.other_lo[:1000]), dtype=np.uint8).reshape(-1, 8)
    assert np.all(words[:, 0] == 0x20) and np.all((words[:, 1:] >= 97) & (words[:, 1:] <= 122))
    assert np.array_equal(library_hash(words), cand.other_h[:1000])


def _hashes(words):
    """{word: hash} of the words of 2..16 bytes"""
    by_len: dict = {}
    for w in words:
        if 2 <= len(w) <= C.K_INLINE:
            by_len.setdefault(len(w), []).append(w)
    out = {}
    for length, ws in by_len.items():
        rows = np.frombuffer(b"".join(ws), dtype=np.uint8).reshape(-1, length)
        out.update(zip(ws, C.hash_rows(rows).tolist()))
    return out


# ---------------------------------------------------------------------- hot_word
@pytest.mark.parametrize("name", C.FAMILIES["hot_word"])
def test_hot_word_sides_of_the_count_field(name):
    c = C.CASES[name]()
    hot, n = c.claims["hot"], c.claims["n"]
    limit = 1 << C.K_CNT_BITS
    assert _oracle_words(name)[hot] == n
    which = name.rsplit("_", 1)[1]
    assert {"below": n == limit - 1, "at": n == limit, "above": n == limit + 1, "double": n == 2 * limit + 3}[which]
    assert (len(hot) <= C.K_INLINE_KEY) == (name.split("_")[2] == "3") and len(hot) in (3, 11)
    assert c.knobs == {"BPE355_STREAM_WG": "1"}
    # the first occurrence alone in the first chunk; every epoch of kEpoch2 chunks holds far more
    # than kKeep2 occurrences and fewer than the 65 536 at which the 16-bit hit mark wraps
    second = c.data.find(hot, 1)
    assert c.data.startswith(hot) and second >= C.K_CHUNK
    epoch = C.K_EPOCH2 * C.K_CHUNK
    body = len(c.data) - second
    assert c.data.count(hot, second, second + epoch) > epoch // (len(hot) + 1)
    assert C.K_KEEP2 * 100 < epoch // (len(hot) + 1) and epoch // len(hot) < 65536 and body > 2 * epoch
    # no other word of the text in the hot word's cache set
    mine = C.cache_set(C.hash_word(hot))
    others = _hashes([w for w in c.plan if w != hot])
    assert len(others) > 2000 and all(C.cache_set(h) != mine for h in others.values())


# ---------------------------------------------------------------------- one_fine_bin
def test_one_fine_bin_overflows_the_reduce_table():
    c = C.CASES["one_fine_bin"]()
    h = _hashes(c.plan)
    assert len(h) == len(c.plan)
    in_bin = [w for w, x in h.items() if C.fine_bin(x) == c.claims["fine"]]
    assert len(in_bin) == c.claims["distinct"] >= C.K_RED_SLOTS + 300
    assert 2000 <= len(h) - len(in_bin) <= 5000
    assert {c.plan[w] for w in in_bin} == {1, 2, 3}
    # shuffled: the bin's words are spread over the whole text
    starts, _lens = _pretokens("one_fine_bin")
    where = np.array([c.data[int(s):int(s) + 8] in set(in_bin) for s in starts])
    quarter = len(where) // 4
    assert all(where[q * quarter:(q + 1) * quarter].mean() > 0.5 for q in range(4))


# ---------------------------------------------------------------------- one_coarse_bin
@pytest.mark.parametrize("name", C.FAMILIES["one_coarse_bin"])
def test_one_coarse_bin_tiles(name):
    c = C.CASES[name]()
    assert set(c.plan.values()) == {1}                               # every occurrence is one record
    h = np.array(list(_hashes(c.plan).values()), dtype=np.uint64)
    assert len(h) == len(c.plan)
    per = np.bincount(C.coarse_bin(h).astype(np.int64), minlength=C.K_COARSE)
    k = c.claims["records"]
    assert per[c.claims["coarse"]] == k and per[0] == 1 and per[C.K_COARSE - 1] == 1
    assert per.sum() == k + 2 and np.count_nonzero(per) == 3         # the other 61 bins get no tile
    want = {"tile": [C.K_L2_TILE], "tile_plus_1": [C.K_L2_TILE, 1],
            "two_tiles_part_plus_1": [C.K_L2_TILE, C.K_L2_TILE, C.K_PART_TILE + 1]}[name[len("one_coarse_bin_"):]]
    assert C.tiles_of(k) == c.claims["tiles"] == want
    per_fine = np.bincount(C.fine_bin(h).astype(np.int64), minlength=C.K_BINS)
    assert per_fine.max() < C.K_RED_SLOTS                            # (fewer words than reduce-table slots per bin)
    assert len(c.data) == 8 * (k + 2)


def test_largest_coarse_case_overflows_a_small_word_table():
    c = C.CASES[C.LARGEST_COARSE]()
    assert len(c.plan) == max(C.COARSE_SIZES.values()) + 2
    # BPE355_WORD_CAP_LOG2=10: the count stops past load 1/2 and reruns with 4x the slots
    cap, grows = 1 << 10, 0
    while len(c.plan) > cap // 2:
        cap, grows = 4 * cap, grows + 1
    assert 3 <= grows <= 8
    assert len(c.data) > 4 * (256 << 10)                             # several 256 KiB windows


# ---------------------------------------------------------------------- dense_two_byte
@pytest.mark.parametrize("name", C.FAMILIES["dense_two_byte"])
def test_dense_two_byte_rate(name):
    c = C.CASES[name]()
    letters, symbols = C.two_byte_characters()
    assert len(letters) + len(symbols) >= 1400 and min(len(letters), len(symbols)) > 300
    assert c.claims["distinct"] == len(c.plan) >= 1400 > 2 * C.K_CACHE2
    assert set(map(len, c.plan)) == {2}
    starts, lens = _pretokens(name)
    assert np.all(lens == 2)
    per_chunk = np.bincount((starts // np.uint64(C.K_CHUNK)).astype(np.int64))
    full = len(c.data) // C.K_CHUNK
    assert full == C.N_DENSE_CHUNKS and 700_000 < len(c.data) < 900_000
    assert np.all(per_chunk[:full] >= 8000) and np.all(per_chunk[:full] == C.K_CHUNK // 2)
    assert per_chunk[0] + 2 * C.K_CACHE2 + 1 == C.K_REC_RESERVE      # the bound, met by a chunk of this text
    # pages turn over: a workgroup's chunks hold more records than a page, at either grid
    wg = int(c.knobs["BPE355_STREAM_WG"])
    assert wg in (1, 4) and (full // wg) * (C.K_CHUNK // 2 - C.K_CACHE2) > C.K_PAGE_RECS


# ---------------------------------------------------------------------- cache_set
def test_cache_set_six_words_in_one_set():
    c = C.CASES["cache_set"]()
    h = _hashes(c.plan)
    assert len(h) == len(c.plan) == 6 + len(c.claims["extras"])
    assert {C.cache_set(x) for x in h.values()} == {c.claims["set"]}
    six = c.claims["six"]
    assert len(set(six)) == 6 and all(len(w) == 8 and c.plan[w] == C.SET_ROUNDS for w in six)
    assert sorted({len(w) for w in c.claims["extras"]}) == list(C.OTHER_LENGTHS) and 8 not in C.OTHER_LENGTHS
    starts, _lens = _pretokens("cache_set")
    seq = [c.data[int(s):int(s) + 8] for s in starts[:12]]
    assert seq == six + six                                          # round-robin


# ---------------------------------------------------------------------- packed_twins
def test_packed_twins_kinds():
    c = C.CASES["packed_twins"]()
    for k in range(2, 41):
        assert c.plan[b"\0" * k] >= 40
    for k in range(1, 21):
        assert c.plan[b"!" + b"\0" * k] >= 40
    nul = [w for w in c.plan if set(w) == {0}]
    assert {len(w) for w in nul} >= {C.K_INLINE_KEY, C.K_INLINE_KEY + 1, C.K_INLINE, C.K_INLINE + 1}
    rows = {len(w): C.pack(np.frombuffer(w, dtype=np.uint8).reshape(1, -1)) for w in nul if len(w) <= C.K_INLINE}
    assert all(int(lo[0]) == 0 and int(hi[0]) == 0 for lo, hi in rows.values())   # told apart by length alone
    assert len({C.hash_word(w) for w in nul if len(w) <= C.K_INLINE}) == C.K_INLINE - 1
    stem = b" abcdefg"
    share = [w for w in c.plan if w.startswith(stem) and len(w) > 8]
    assert sorted({len(w) for w in share}) == list(range(9, 17)) and len(share) == 16 and stem in c.plan
    byte1 = [w for w in c.plan if len(w) == 16 and w[:1] == b" " and w[2:] == b"bcdefghijklmno"]
    assert len(byte1) == 11                                          # b..k, and the stem's own 16-byte word


# ---------------------------------------------------------------------- long_distinct
def test_long_distinct_overflows_the_long_table():
    c = C.CASES["long_distinct"]()
    assert c.knobs == {"BPE355_STREAM_WG": "1", "BPE355_LONG_SEG": str(C.LONG_SEG)}
    longs = {w for w in c.plan if len(w) > C.K_INLINE and w != C.WS_RUN}
    assert len(longs) == c.claims["distinct"] >= C.K_LONG_SLOTS + 1000
    assert min(map(len, longs)) == 17 and max(map(len, longs)) == 60
    assert {c.plan[w] for w in longs} == {1, 2, 3}
    assert 20 <= len(C.WS_RUN) <= 30 and c.plan[C.WS_RUN] == 70_000
    # the one workgroup's segment (the first LONG_SEG long pre-tokens) holds every distinct word
    starts, lens = _pretokens("long_distinct")
    long_at = starts[lens > C.K_INLINE][:C.LONG_SEG]
    long_len = lens[lens > C.K_INLINE][:C.LONG_SEG]
    head = {c.data[int(s):int(s) + int(n)] for s, n in zip(long_at, long_len)}
    assert c.claims["head"] < C.LONG_SEG and longs < head and len(head) > C.K_LONG_SLOTS
    assert (2 << 20) < len(c.data) < (6 << 20)                       # more than one 1 MiB file segment
