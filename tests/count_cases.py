"""The word counter at the capacity edges of its record aggregation: texts constructed for every
threshold of csrc/count.hip and of table_add (csrc/stage.h) that random text does not reach below
bench scale, and the plain-numpy restatements that show (tests/test_count_cases.py, on the CPU)
that a text reaches what it claims.  tests/test_gpu_count_edges.py runs them on the device.

What the counter derives from a short word's hash h = short_hash(lo, hi, len) (lo, hi: the word's
bytes packed little-endian, pack_word):
  coarse bin   h >> 58                 level 1 of the record partition (kCoarse = 64 bins)
  fine bin     h >> 52                 the bin k_rec_reduce sums in one LDS table (kBins = 4096)
  cache set    (h >> 40) & 510         the 2-way set of k_count2's LDS word cache (kCache2 = 512)
  reduce slot  (h >> 20) & 4095        the first slot probed in k_rec_reduce's LDS table
short_hash is restated here and pinned to the library's own by bpe_short_hash_host.

Candidate words are " " + 7 lowercase letters (8 bytes, one pre-token each, lo = the 8 bytes,
hi = 0) from a fixed seed; 20 M of them are hashed once per process (candidates()), of which the
fullest fine bin outside coarse bins 0 and 63, its whole coarse bin and the first 2^18 are kept.

A case holds its family, the text (bytes), the knobs it is meant for (environment variables of the
counter's test knobs) and its planned word multiset {pre-token: count}, one-byte pre-tokens
included: an expectation that owes nothing to the oracle.

Families (CASES):
  hot_word        one word N times through one workgroup (BPE355_STREAM_WG=1), N on both sides of
                  1 << kCntBits, where a flushed cache entry stops fitting a record's count field
                  and goes to table_add with a large count; a 3-byte word (inline key) and an
                  11-byte one (offset key).  The word's first occurrence stands alone in the first
                  chunk, so one thread claims its cache entry without a race and every later
                  occurrence hits it: the entry is flushed once, with count N.  No other word of
                  the text shares its cache set.
  one_fine_bin    kRedSlots + 300 distinct words of one fine bin, 1-3 times each: k_rec_reduce's
                  LDS table cannot hold them, the rest go to the global table from the record loop
  one_coarse_bin  all-distinct words of one coarse bin, once each: exactly kL2Tile, kL2Tile + 1
                  and 2 kL2Tile + kPartTile + 1 records there (1, 2, 3 level-2 tiles, the last of
                  1 and of kPartTile + 1 records), one record each in coarse bins 0 and 63, none
                  in the other 61; every occurrence is one record
  dense_two_byte  alternating 2-byte letters and 2-byte symbols: 8192 pre-tokens of 2 bytes per
                  chunk, the rate kRecReserve is written for, with more distinct words than the
                  cache has entries; for 1 and 4 workgroups, so that pages turn over
  cache_set       six words of one cache set in round-robin, with words of other lengths in the set
  packed_twins    words whose packed bytes are equal or nearly so: NUL runs of 2..40 bytes, "!" and
                  1..20 NULs, words of 9..16 bytes sharing their first 8, words differing in byte 1
  long_distinct   kLongSlots + 1000 distinct words of 17..60 bytes, 1-3 times each, all among the
                  first BPE355_LONG_SEG=8192 long pre-tokens of the one workgroup's segment, and a
                  run of 24 spaces 70 000 times

Building every case takes 2.4 s on the CPU, 1.8 s of it the candidate table (measured, one core);
tests/test_count_cases.py takes 6 to 8 s with the oracle's runs.
"""
from __future__ import annotations

import collections
import functools
import unicodedata

import numpy as np

# ---------------------------------------------------------------------- constants, as the source has them
K_CHUNK = 16384              # kChunk      csrc/stage.h
K_HALO = 1024                # kHalo       csrc/stage.h
K_INLINE_KEY = 7             # kInlineKey  csrc/stage.h
K_INLINE = 16                # kInline     csrc/stage.h
K_PAGE_RECS = 65536          # kPageRecs   csrc/count.h
K_COARSE_BITS = 6            # kCoarseBits csrc/count.h
K_COARSE = 1 << K_COARSE_BITS
K_CACHE2 = 512               # kCache2     csrc/count.hip
K_EPOCH2 = 4                 # kEpoch2
K_KEEP2 = 2                  # kKeep2
K_CNT_BITS = 19              # kCntBits
K_REC_RESERVE = K_CHUNK // 2 + 1 + 2 * K_CACHE2   # kRecReserve
K_BIN_BITS = 12              # kBinBits
K_BINS = 1 << K_BIN_BITS
K_PART_TILE = 4096           # kPartTile
K_L2_TILE = 65536            # kL2Tile
K_RED_SLOTS = 4096           # kRedSlots
K_RED_PROBE = 64             # kRedProbe
K_LONG_SLOTS = 2048          # kLongSlots
K_LONG_PROBE = 16            # kLongProbe

# name here -> (file under transformer-lm_amd/csrc, name there)
SOURCE_CONSTANTS = {
    "K_CHUNK": ("stage.h", "kChunk"), "K_HALO": ("stage.h", "kHalo"), "K_INLINE_KEY": ("stage.h", "kInlineKey"),
    "K_INLINE": ("stage.h", "kInline"), "K_PAGE_RECS": ("count.h", "kPageRecs"),
    "K_COARSE_BITS": ("count.h", "kCoarseBits"), "K_COARSE": ("count.h", "kCoarse"),
    "K_CACHE2": ("count.hip", "kCache2"), "K_EPOCH2": ("count.hip", "kEpoch2"), "K_KEEP2": ("count.hip", "kKeep2"),
    "K_CNT_BITS": ("count.hip", "kCntBits"), "K_REC_RESERVE": ("count.hip", "kRecReserve"),
    "K_BIN_BITS": ("count.hip", "kBinBits"), "K_BINS": ("count.hip", "kBins"),
    "K_PART_TILE": ("count.hip", "kPartTile"), "K_L2_TILE": ("count.hip", "kL2Tile"),
    "K_RED_SLOTS": ("count.hip", "kRedSlots"), "K_RED_PROBE": ("count.hip", "kRedProbe"),
    "K_LONG_SLOTS": ("count.hip", "kLongSlots"), "K_LONG_PROBE": ("count.hip", "kLongProbe"),
}

N_CANDIDATES = 20_000_000
SEED = 355
LONG_SEG = 8192              # BPE355_LONG_SEG of the long_distinct case


# ---------------------------------------------------------------------- the hash, restated
_M1 = np.uint64(0x9E3779B97F4A7C15)
_M2 = np.uint64(0xD6E8FEB86659FD93)
_S32 = np.uint64(32)


def short_hash(lo, hi, length: int) -> np.ndarray:
    """stage.h short_hash on arrays of packed words (uint64 arithmetic wraps)"""
    lo = np.atleast_1d(np.asarray(lo, dtype=np.uint64))
    hi = np.atleast_1d(np.asarray(hi, dtype=np.uint64))
    z = lo ^ ((hi ^ np.uint64(length)) * _M1)
    z = z ^ (z >> _S32)
    z = z * _M2
    return z ^ (z >> _S32)


def pack(words: np.ndarray):
    """pack_word: (n, len) bytes -> (lo, hi); byte i is bits 8 i of lo for i < 8, of hi beyond"""
    n, length = words.shape
    assert 1 <= length <= K_INLINE
    padded = np.zeros((n, 16), dtype=np.uint8)
    padded[:, :length] = words
    both = padded.view("<u8")
    return both[:, 0].copy(), both[:, 1].copy()


def hash_rows(words: np.ndarray) -> np.ndarray:
    lo, hi = pack(words)
    return short_hash(lo, hi, words.shape[1])


def hash_word(word: bytes) -> int:
    return int(hash_rows(np.frombuffer(word, dtype=np.uint8).reshape(1, -1))[0])


def coarse_bin(h):
    return h >> np.uint64(64 - K_COARSE_BITS) if isinstance(h, np.ndarray) else h >> (64 - K_COARSE_BITS)


def fine_bin(h):
    return h >> np.uint64(64 - K_BIN_BITS) if isinstance(h, np.ndarray) else h >> (64 - K_BIN_BITS)


def cache_set(h):
    if isinstance(h, np.ndarray):
        return (h >> np.uint64(40)) & np.uint64(K_CACHE2 - 2)
    return (h >> 40) & (K_CACHE2 - 2)


def reduce_slot(h):
    if isinstance(h, np.ndarray):
        return (h >> np.uint64(20)) & np.uint64(K_RED_SLOTS - 1)
    return (h >> 20) & (K_RED_SLOTS - 1)


def tiles_of(records: int):
    """k_rec_tiles: the level-2 tile lengths of a coarse bin of that many records"""
    return [min(K_L2_TILE, records - a) for a in range(0, records, K_L2_TILE)]


# ---------------------------------------------------------------------- candidates
class Candidates:
    """8-byte words " xxxxxxx" as their packed lo (hi = 0), with their hashes"""

    def __init__(self, fine, coarse_lo, coarse_h, other_lo, other_h, fullest):
        self.fine = fine                 # the target fine bin
        self.coarse = fine >> K_COARSE_BITS
        self.coarse_lo, self.coarse_h = coarse_lo, coarse_h     # every distinct candidate of that coarse bin
        self.other_lo, self.other_h = other_lo, other_h         # the first 2^18 candidates, distinct
        self.fullest = fullest           # candidates in the target fine bin, duplicates included


def _unique(lo, h):
    _u, first = np.unique(lo, return_index=True)
    first.sort()                         # generation order kept
    return lo[first], h[first]


@functools.lru_cache(maxsize=None)
def candidates() -> Candidates:
    rng = np.random.default_rng(SEED)
    block = 2_000_000
    los, fines = [], []
    for _ in range(N_CANDIDATES // block):
        b = np.empty((block, 8), dtype=np.uint8)
        b[:, 0] = 0x20
        b[:, 1:] = rng.integers(97, 123, (block, 7), dtype=np.uint8)
        lo = b.view("<u8").ravel()
        los.append(lo)
        fines.append((short_hash(lo, 0, 8) >> np.uint64(64 - K_BIN_BITS)).astype(np.uint16))
    lo, fine = np.concatenate(los), np.concatenate(fines)
    del los, fines
    per_fine = np.bincount(fine, minlength=K_BINS)
    per_fine[:K_COARSE] = 0              # coarse bins 0 and 63 are kept for the lone records
    per_fine[-K_COARSE:] = 0
    target = int(per_fine.argmax())
    keep = lo[(fine >> K_COARSE_BITS) == (target >> K_COARSE_BITS)]
    coarse_lo, coarse_h = _unique(keep, short_hash(keep, 0, 8))
    other = lo[:1 << 18]
    other_lo, other_h = _unique(other, short_hash(other, 0, 8))
    return Candidates(target, coarse_lo, coarse_h, other_lo, other_h, int(per_fine[target]))


def text_of(lo: np.ndarray) -> bytes:
    """the 8-byte words, end to end"""
    return lo.astype("<u8").tobytes()


def word_of(lo) -> bytes:
    return int(lo).to_bytes(8, "little")


def plan_of(lo: np.ndarray) -> dict:
    u, c = np.unique(lo, return_counts=True)
    raw = u.astype("<u8").tobytes()
    return {raw[8 * i:8 * i + 8]: int(n) for i, n in enumerate(c.tolist())}


def _add(plan: dict, other: dict) -> dict:
    for w, n in other.items():
        plan[w] = plan.get(w, 0) + n
    return plan


class Case:
    def __init__(self, name, family, data, plan, knobs=None, **claims):
        self.name, self.family = name, family
        self.data = data
        self.plan = plan                 # {pre-token: count}, one-byte pre-tokens included
        self.knobs = dict(knobs or {})   # the test knobs the case is meant for, beside the pool
        self.claims = claims

    def words(self) -> dict:
        """the plan as the device reports it: pre-tokens of two bytes and more"""
        return {w: n for w, n in self.plan.items() if len(w) > 1}


# ---------------------------------------------------------------------- hot_word
HOT_WORDS = {3: b" AB", 11: b" ABCDEFGHIJ"}   # (upper case: inside no candidate)
HOT_COUNTS = {"below": (1 << K_CNT_BITS) - 1, "at": 1 << K_CNT_BITS, "above": (1 << K_CNT_BITS) + 1,
              "double": (1 << (K_CNT_BITS + 1)) + 3}
HOT_EVERY = 211              # a sprinkled word behind every 211th occurrence


def _hot_word(length: int, which: str) -> Case:
    C = candidates()
    hot, n = HOT_WORDS[length], HOT_COUNTS[which]
    hot_set = cache_set(hash_word(hot))
    others = C.other_lo[cache_set(C.other_h) != np.uint64(hot_set)]
    n_fill = (K_CHUNK + K_HALO) // 8 + 1         # the second occurrence starts past the first chunk
    fill, rest = others[:n_fill], others[n_fill:]
    groups = (n - 1) // HOT_EVERY
    sprinkle = rest[np.arange(groups) % 5000]    # (5000 distinct words, most of them several times)
    group = hot * HOT_EVERY
    raw = text_of(sprinkle)
    body = b"".join(group + raw[8 * i:8 * i + 8] for i in range(groups)) + hot * ((n - 1) - groups * HOT_EVERY)
    plan = _add(plan_of(fill), plan_of(sprinkle))
    plan[hot] = n
    return Case(f"hot_word_{length}_{which}", "hot_word", hot + text_of(fill) + body, plan,
                {"BPE355_STREAM_WG": "1"}, hot=hot, n=n)


# ---------------------------------------------------------------------- one_fine_bin
N_FINE = K_RED_SLOTS + 300


def _one_fine_bin() -> Case:
    C = candidates()
    rng = np.random.default_rng(SEED + 1)
    mine = C.coarse_lo[fine_bin(C.coarse_h) == np.uint64(C.fine)][:N_FINE]
    assert len(mine) == N_FINE, len(mine)
    elsewhere = C.other_lo[fine_bin(C.other_h) != np.uint64(C.fine)][:3000]
    lo = np.concatenate([np.repeat(mine, rng.integers(1, 4, len(mine))), elsewhere])
    lo = lo[rng.permutation(len(lo))]
    return Case("one_fine_bin", "one_fine_bin", text_of(lo), plan_of(lo), {"BPE355_STREAM_WG": "2"},
                fine=C.fine, distinct=N_FINE)


# ---------------------------------------------------------------------- one_coarse_bin
COARSE_SIZES = {"tile": K_L2_TILE, "tile_plus_1": K_L2_TILE + 1, "two_tiles_part_plus_1": 2 * K_L2_TILE + K_PART_TILE + 1}
LARGEST_COARSE = "one_coarse_bin_two_tiles_part_plus_1"


def _one_coarse_bin(which: str) -> Case:
    C = candidates()
    k = COARSE_SIZES[which]
    rng = np.random.default_rng(SEED + 2)
    assert len(C.coarse_lo) >= k
    oc = coarse_bin(C.other_h)
    ends = [C.other_lo[oc == np.uint64(b)][0] for b in (0, K_COARSE - 1)]
    lo = np.concatenate([C.coarse_lo[:k], np.array(ends, dtype=np.uint64)])
    lo = lo[rng.permutation(len(lo))]
    return Case(f"one_coarse_bin_{which}", "one_coarse_bin", text_of(lo), plan_of(lo), {"BPE355_STREAM_WG": "2"},
                coarse=C.coarse, records=k, tiles=tiles_of(k))


# ---------------------------------------------------------------------- dense_two_byte
def two_byte_characters():
    """(letters, symbols) of U+0080..U+07FF: assigned characters, the symbols neither letters,
    numbers, white space nor controls"""
    letters, symbols = [], []
    for cp in range(0x80, 0x800):
        c = chr(cp)
        cat = unicodedata.category(c)
        if cat[0] == "L":
            letters.append(c)
        elif cat[0] not in "NZ" and cat not in ("Cc", "Cn") and not c.isspace():
            symbols.append(c)
    return letters, symbols


N_DENSE_CHUNKS = 49


def _dense_two_byte(wg: int) -> Case:
    letters, symbols = two_byte_characters()
    rng = np.random.default_rng(SEED + 3)
    n = N_DENSE_CHUNKS * K_CHUNK // 2 + 1500     # 49 full chunks and a partial one
    codes = np.empty(n, dtype=np.uint16)
    codes[0::2] = np.array([ord(c) for c in letters], dtype=np.uint16)[rng.integers(0, len(letters), (n + 1) // 2)]
    codes[1::2] = np.array([ord(c) for c in symbols], dtype=np.uint16)[rng.integers(0, len(symbols), n // 2)]
    two = np.empty((n, 2), dtype=np.uint8)       # 110xxxxx 10xxxxxx
    two[:, 0] = 0xC0 | (codes >> 6)
    two[:, 1] = 0x80 | (codes & 0x3F)
    u, c = np.unique(codes, return_counts=True)
    plan = {chr(int(cp)).encode("utf-8"): int(k) for cp, k in zip(u, c)}
    return Case(f"dense_two_byte_wg{wg}", "dense_two_byte", two.tobytes(), plan, {"BPE355_STREAM_WG": str(wg)},
                distinct=len(u))


# ---------------------------------------------------------------------- cache_set
OTHER_LENGTHS = (4, 6, 11, 16)
SET_ROUNDS = 4000


def _letter_words(length: int, n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    b = np.empty((n, length), dtype=np.uint8)
    b[:, 0] = 0x20
    b[:, 1:] = rng.integers(97, 123, (n, length - 1), dtype=np.uint8)
    return np.unique(b, axis=0)


def _cache_set() -> Case:
    C = candidates()
    sets = cache_set(C.other_h)
    target = int(sets[0])
    six = C.other_lo[sets == np.uint64(target)][:6]
    assert len(six) == 6
    extras = []
    for length in OTHER_LENGTHS:
        w = _letter_words(length, 20000, SEED + 10 + length)
        same = w[cache_set(hash_rows(w)) == np.uint64(target)][:3]
        assert len(same) == 3, (length, len(same))
        extras += [bytes(r) for r in same]
    six_words = [word_of(x) for x in six]
    round_ = b"".join(six_words)
    parts, plan = [], collections.Counter()
    for r in range(SET_ROUNDS):
        parts.append(round_)
        if r % 7 == 6:
            e = extras[(r // 7) % len(extras)]
            parts.append(e)
            plan[e] += 1
    for w in six_words:
        plan[w] = SET_ROUNDS
    return Case("cache_set", "cache_set", b"".join(parts), dict(plan), {"BPE355_STREAM_WG": "2"},
                set=target, six=six_words, extras=extras)


# ---------------------------------------------------------------------- packed_twins
def _packed_twins() -> Case:
    rng = np.random.default_rng(SEED + 4)
    items = []                                   # (piece of text, its pre-tokens)
    for k in range(2, 41):                       # a digit before a NUL run: neither joins a neighbour
        items.append((b"7" + b"\0" * k, [b"7", b"\0" * k]))
    for k in range(1, 21):
        items.append((b"7!" + b"\0" * k, [b"7", b"!" + b"\0" * k]))
    stem = b" abcdefg"
    for k in range(1, 9):                        # 9..16 bytes sharing lo; two of each length
        for tail in (b"hijklmno"[:k], b"hijklmnp"[:k - 1] + b"z"):
            items.append((stem + tail, [stem + tail]))
    items.append((stem, [stem]))
    for c in b"bcdefghijk":                      # differing in byte 1 only, at 3, 8, 12 and 16 bytes
        for rest in (b"z", b"bcdefg", b"bcdefghijk", b"bcdefghijklmno"):
            w = b" " + bytes([c]) + rest
            items.append((w, [w]))
    plan, pieces = collections.Counter(), []
    for piece, tokens in items:
        reps = int(rng.integers(1, 6)) * 40
        pieces += [piece] * reps
        for t in tokens:
            plan[t] += reps
    order = rng.permutation(len(pieces))
    return Case("packed_twins", "packed_twins", b"".join(pieces[i] for i in order), dict(plan), {"BPE355_STREAM_WG": "2"})


# ---------------------------------------------------------------------- long_distinct
N_LONG = K_LONG_SLOTS + 1000
WS_RUN = b" " * 24
WS_TIMES = 70_000
WS_UNIT = WS_RUN + b" cd ef"                     # -> the run, " cd", " ef" (a safe split point between them)


def _long_distinct() -> Case:
    rng = np.random.default_rng(SEED + 5)
    words = set()
    while len(words) < N_LONG:
        k = int(rng.integers(17, 61))
        words.add(b" " + bytes(rng.integers(97, 123, k - 1, dtype=np.uint8)))
    words = sorted(words)
    plan = collections.Counter()
    occ = []
    for w in words:
        reps = int(rng.integers(1, 4))
        plan[w] = reps
        occ += [w] * reps
    order = rng.permutation(len(occ))
    parts, runs = [], 0
    for j, i in enumerate(order):                # every distinct word first, a run behind every 8th
        parts.append(occ[i])
        if j % 8 == 7:
            parts.append(WS_UNIT)
            runs += 1
    parts.append(WS_UNIT * (WS_TIMES - runs))
    plan[WS_RUN] = WS_TIMES
    plan[b" cd"] = WS_TIMES
    plan[b" ef"] = WS_TIMES
    return Case("long_distinct", "long_distinct", b"".join(parts), dict(plan),
                {"BPE355_STREAM_WG": "1", "BPE355_LONG_SEG": str(LONG_SEG)}, distinct=N_LONG, head=len(occ) + runs)


# ---------------------------------------------------------------------- all of them
def _named(f, *args):
    g = functools.lru_cache(maxsize=None)(lambda: f(*args))
    return g


CASES = {}
for _len in HOT_WORDS:
    for _which in HOT_COUNTS:
        CASES[f"hot_word_{_len}_{_which}"] = _named(_hot_word, _len, _which)
CASES["one_fine_bin"] = _named(_one_fine_bin)
for _which in COARSE_SIZES:
    CASES[f"one_coarse_bin_{_which}"] = _named(_one_coarse_bin, _which)
for _wg in (1, 4):
    CASES[f"dense_two_byte_wg{_wg}"] = _named(_dense_two_byte, _wg)
CASES["cache_set"] = _named(_cache_set)
CASES["packed_twins"] = _named(_packed_twins)
CASES["long_distinct"] = _named(_long_distinct)

FAMILIES = {"hot_word": [n for n in CASES if n.startswith("hot_word")],
            "one_fine_bin": ["one_fine_bin"],
            "one_coarse_bin": [n for n in CASES if n.startswith("one_coarse_bin")],
            "dense_two_byte": [n for n in CASES if n.startswith("dense_two_byte")],
            "cache_set": ["cache_set"], "packed_twins": ["packed_twins"], "long_distinct": ["long_distinct"]}
TRAIN_CASES = ["one_fine_bin", LARGEST_COARSE, "dense_two_byte_wg4", "long_distinct"]
TRAIN_VOCAB = 600
