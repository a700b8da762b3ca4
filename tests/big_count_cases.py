"""Pre-counted training inputs whose word counts lie between 2^31 and the documented limit
(the sum over all words of count * length below 2^62: include/bpe355.h),
and the exact reference they are trained against.

A WordCounter takes {word: count} directly (add_counts, train_bpe_word_counts), so counts no text
could reach cost nothing to make.  What they exercise on the device: the merge's 32-bit LDS cells
and their switch to the 64-bit global cells when the round's best count reaches 2^32
(csrc/train_merge.h `narrow`, train_select.h DeltaSinkN), and 64-bit counts in every other stage
(the pair histogram, the log2 bins and thresholds of the candidate rebuild, the order of
candidates, the apply's deltas, compaction, the pair table's rehash, the long-word table).

train_counts(counts, vocab_size, specials, on_round) is the reference: the round loop of
oracle/cpu_ref.py (reference train.py:183-228, vocab.py:2-34) restated over {bytes: int}.  Python
ints make it exact at any magnitude; the C oracle counts in 64 bits and reads text, so it only
serves where a case is a text's own counts times one factor (scaling every count by the same
factor keeps the order of pairs and every tie, so the merges are those of the unscaled text).

The cases, each {bytes: int}:

  scaled(text_case, k)    the counts of a text times k: 2^32 (counts differ only above bit 32),
                          2^32 + 1 (equal low and high words), 2^33 - 1 (a third mix).  The texts:
                          "synth", and the three deep-tie kinds of tests/tie_cases.py, whose ties
                          then sit at counts with colliding low words
  crossing()              "synth" times 2^CROSSING_SHIFT: the best count falls from above 2^32
                          through [2^31, 2^32) to below 2^31, with at least 100 rounds in each
  mixed_magnitudes(seed)  "synth" with a per-word factor from {1, 2^12, 2^24, 2^31 + 5}: pair
                          counts sum words of very different sizes (only train_counts applies)
  boundary(V)             about 300 words " xab" + suffix whose counts sum to exactly V, in every
                          slot class and the long table: rounds 0-2 are (x,a), (xa,b), (" ",xab)
                          with count exactly V each, the neighbour cells of these merges sum to
                          exactly V over words of different workgroups
  one_block(V)            the same three rounds, but V lies in two 4- and 5-byte words that one
                          workgroup rewrites: one 32-bit LDS cell receives exactly V
  grows_pair_table()      "nul" times 2^33 - 1, trained to GROW_VOCAB: more tokens than a first pair
                          table of 2^18 slots allows, so the table is rehashed at these counts
  near_limit()            "synth" times the largest factor that keeps the weight <= 2^62 - 1

The generator is the integer-only SplitMix64 of tests/golden/synth_text.py.
"""
from __future__ import annotations

import functools

import synth_text
import tie_cases
from oracle import oracle
from synth_text import SplitMix64

WEIGHT_LIMIT = 1 << 62             # accepted: sum of count * length < 2^62
FACTORS = ((1 << 32), (1 << 32) + 1, (1 << 33) - 1)
SYNTH = (5, 100_000, "mixed")      # synth_text.generate arguments
TEXT_CASES = ("synth",) + tie_cases.KINDS
VOCAB = 1200                       # scaled, crossing, mixed_magnitudes, near_limit: compactions occur
BOUNDARY_VOCAB = 300
EXHAUST_VOCAB = 66_000             # u32 ids; boundary(V, EXHAUST_WORDS) runs out of pairs long before
EXHAUST_WORDS = 23                 # " xab" and two or three words of each other length
GROW_VOCAB = 2300                  # see grows_pair_table()
CROSSING_SHIFT = 25                # see crossing()
MAGNITUDES = (1, 1 << 12, 1 << 24, (1 << 31) + 5)
BOUNDARY_VS = ((1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1,
               (1 << 61) // 80)
# " xab" + suffix: 4, 5, 7 | 9, 13 | 17, 24 | 33, 44 | 65, 74 bytes
BOUNDARY_SUFFIXES = (0, 1, 3, 5, 9, 13, 20, 29, 40, 61, 70)
BOUNDARY_WORDS = 300
_LETTERS = "cdefghijklmnopqrstuvwyz"   # no "x", "a", "b"


def train_counts(counts, vocab_size, specials=(), on_round=None):
    """(vocab, merges) of the reference trainer on the pre-token counts {bytes: int}: per round
    the max over all pairs by (count, pair), the words holding it rewritten left to right with
    the neighbour counts updated on the partly rewritten word, the best pair popped; the vocab
    is the specials, the 256 bytes, then each merged token, deduplicated.  A word equal to a
    special token is dropped (train.py:25).  on_round(pairs, best) is called before each
    rewrite, as cpu_ref.train calls it."""
    vocab_list, present = [], set()
    for tok in [s.encode("utf-8") for s in specials] + [bytes([i]) for i in range(256)]:
        if tok not in present:
            present.add(tok)
            vocab_list.append(tok)
    skip = {s.encode("utf-8") for s in specials}
    words, freq = [], []
    for w, c in counts.items():
        if w in skip or not c:
            continue
        words.append([bytes([b]) for b in w])
        freq.append(int(c))
    pairs: dict = {}
    where: dict = {}
    for wi, w in enumerate(words):
        c = freq[wi]
        for p in zip(w, w[1:]):
            pairs[p] = pairs.get(p, 0) + c
            where.setdefault(p, set()).add(wi)
    merges = []
    for _ in range(max(0, vocab_size - len(vocab_list))):
        if not pairs:
            break
        best = max(pairs, key=lambda p: (pairs[p], p))
        if on_round is not None:
            on_round(pairs, best)
        a, b = best
        new = a + b
        if new not in present:
            present.add(new)
            vocab_list.append(new)
        for wi in list(where.get(best, ())):
            w, c = words[wi], freq[wi]
            i = 0
            while i < len(w) - 1:
                if w[i] == a and w[i + 1] == b:
                    if i > 0:
                        left = (w[i - 1], a)
                        pairs[left] = pairs.get(left, 0) - c
                        pairs[(w[i - 1], new)] = pairs.get((w[i - 1], new), 0) + c
                    if i < len(w) - 2:
                        right = (b, w[i + 2])
                        pairs[right] = pairs.get(right, 0) - c
                        pairs[(new, w[i + 2])] = pairs.get((new, w[i + 2]), 0) + c
                    w[i] = new
                    del w[i + 1]
                    if i > 0:
                        where.setdefault((w[i - 1], new), set()).add(wi)
                    if i < len(w) - 1:
                        where.setdefault((new, w[i + 1]), set()).add(wi)
                i += 1
        pairs.pop(best)
        where.pop(best, None)
        merges.append(best)
    return dict(enumerate(vocab_list)), merges


def tops(counts, vocab_size, specials=()):
    """(vocab, merges, [the best pair's count in each round]) of train_counts."""
    out = []
    vocab, merges = train_counts(counts, vocab_size, specials, lambda pairs, best: out.append(pairs[best]))
    return vocab, merges, out


def weight(counts) -> int:
    """What the library bounds: the sum of count * length over the words it keeps (>= 2 bytes)."""
    return sum(c * len(w) for w, c in counts.items() if len(w) >= 2)


def n_pretokens(counts) -> int:
    """The library's n_pretokens for these counts: words under 2 bytes carry no pair and are dropped."""
    return sum(c for w, c in counts.items() if len(w) >= 2)


@functools.lru_cache(maxsize=None)
def text_bytes(text_case: str) -> bytes:
    if text_case == "synth":
        return synth_text.generate(*SYNTH).encode("utf-8")
    return tie_cases.case(0, text_case, tie_cases.SCALED_WORDS).encode("utf-8")


@functools.lru_cache(maxsize=None)
def _base(text_case: str):
    # (a file's bytes are decoded, newlines translated, before they are pre-tokenized)
    return tuple(oracle.word_counts(oracle.decode_text(text_bytes(text_case)), []).items())


def base_counts(text_case: str = "synth") -> dict:
    return dict(_base(text_case))


def scaled(text_case: str, k: int) -> dict:
    return {w: c * k for w, c in _base(text_case)}


def crossing(shift: int = CROSSING_SHIFT) -> dict:
    """CROSSING_SHIFT is chosen so that at VOCAB the best count is >= 2^32 in at least 100 rounds,
    in [2^31, 2^32) in at least 100 and below 2^31 in at least 100 (tests/test_big_count_cases.py
    counts them through on_round)."""
    return scaled("synth", 1 << shift)


def grows_pair_table() -> dict:
    """The "nul" text times 2^33 - 1, to be trained to GROW_VOCAB: 2044 rounds, the best count still
    2^33 - 1 in the last.  The batched loop keeps room in the pair table for 4 * 16 * (tokens + 16)
    new keys per trip, so a first table of 2^18 slots (BPE355_PAIR_CAP_LOG2=18, the smallest) must
    grow once the tokens pass 2032, whatever the number of pairs: k_rehash then moves live counts
    that are all multiples of 2^33 - 1.  (At VOCAB = 1200 no case here makes that table grow.  The
    factor is not 2^32 + 1: the low word of m * (2^32 + 1) is m, so counts cut to 32 bits would
    keep their order and every tie; the low word of m * (2^33 - 1) is -m.)"""
    return scaled("nul", (1 << 33) - 1)


def mixed_magnitudes(seed: int = 0) -> dict:
    r = SplitMix64(0xB16C0 + seed)
    return {w: c * MAGNITUDES[r.below(len(MAGNITUDES))] for w, c in _base("synth")}


def _suffix(r: SplitMix64, n: int) -> str:
    return "".join(_LETTERS[r.below(len(_LETTERS))] for _ in range(n))


def boundary(V: int, n_words: int = BOUNDARY_WORDS) -> dict:
    """Every word but " xab" itself gets V * r / sum(r) for a random r in 1..1000, " xab" the rest:
    the counts sum to exactly V and, of the 300, no word has more than V / 100, so a pair inside
    the random suffixes (23 letters: a pair recurs a few times over all words) stays far below V.
    n_words = EXHAUST_WORDS: the first of the same words, few enough to train until no pair is left
    (some 1200 merges, those of pairs whose count fell to zero included) in well under a second of
    plain Python."""
    r = SplitMix64(0xB0DA)
    words = [b" xab"]               # (the one word without a suffix)
    tries = 0
    while len(words) < n_words:   # the lengths in turn (there are only 23 one-letter suffixes)
        w = (" xab" + _suffix(r, BOUNDARY_SUFFIXES[1 + tries % (len(BOUNDARY_SUFFIXES) - 1)])).encode()
        tries += 1
        if w not in words:
            words.append(w)
    share = [1 + r.below(1000) for _ in words]
    total = sum(share)
    out = {w: V * s // total for w, s in zip(words, share)}
    out[b" xab"] += V - sum(out.values())
    assert sum(out.values()) == V and all(c > 0 for c in out.values()) and len(out) == len(words)
    return out


def one_block(V: int) -> dict:
    """V in " xab" and " xabc" (one slot class, neighbouring slots: one workgroup rewrites both, so
    its LDS cell for the left neighbour " " receives exactly V in two adds whose low words carry),
    beside 40 words of small counts over other letters that keep the run going."""
    r = SplitMix64(0x0B10C)
    out = {b" xab": V - V // 3, b" xabc": V // 3}
    while len(out) < 42:
        w = (" " + _suffix(r, 2 + r.below(70))).encode()
        if w not in out:
            out[w] = 1 + r.below(1000)
    return out


def near_limit() -> dict:
    base = dict(_base("synth"))
    return {w: c * ((WEIGHT_LIMIT - 1) // weight(base)) for w, c in base.items()}


def class_of(n_ids: int) -> int:
    """The slot class of a word of n_ids ids (csrc/train_state.h class_for); 4: the long table."""
    return 0 if n_ids <= 7 else 1 if n_ids <= 15 else 2 if n_ids <= 31 else 3 if n_ids <= 63 else 4


def common_word() -> str:
    """The most frequent multi-byte word of "synth" that is valid UTF-8: a special token equal to
    it takes it out of the counts (train.py:25)."""
    c, w = max((c, w) for w, c in _base("synth") if len(w) >= 3 and w.isascii())
    return w.decode("ascii")


def parity_cases():
    """{id: (builder of the counts, vocab size, special tokens)}: what the device is trained on.
    The scaled "synth" cases carry no special, one that is no word, and one that is a word."""
    eot = "<|endoftext|>"
    sp = {FACTORS[0]: (), FACTORS[1]: (eot,), FACTORS[2]: (eot, common_word())}
    out = {}
    for t in TEXT_CASES:
        for k in FACTORS:
            out[f"scaled-{t}-{k:#x}"] = (functools.partial(scaled, t, k), VOCAB, sp[k] if t == "synth" else ())
    out["crossing"] = (crossing, VOCAB, ())
    out["mixed_magnitudes"] = (mixed_magnitudes, VOCAB, ())
    for V in BOUNDARY_VS:
        out[f"boundary-{V:#x}"] = (functools.partial(boundary, V), BOUNDARY_VOCAB, ())
    for V in BOUNDARY_VS:
        out[f"one_block-{V:#x}"] = (functools.partial(one_block, V), BOUNDARY_VOCAB, ())
    out["near_limit"] = (near_limit, VOCAB, ())
    return out
