"""Training inputs whose words sit on both sides of every word-length boundary of the merge loop.

csrc/train.hip keeps a word of n token ids in a slot of 8, 16, 32 or 64 ids (class_for: n <= 7,
<= 15, <= 31, <= 63) or, past 63 ids, in the CSR table of long words, and rewrites each of these
by other code (rewrite_slot_members in registers for classes 0-2, rewrite_slot from memory for
class 3, the serial rewrite_word for long words); compact() moves a word down as it shrinks.  A
word starts with one id per byte of its pre-token, leading space included, so the pre-token byte
lengths below are the id counts the words start with.

case(kind, seed): for every length of LENGTHS three distinct words (fewer where the kind has
fewer: "runs" has two one-letter words), each repeated 1, 2, 3, 5 or 40 times, shuffled, every
word behind one space.  The kinds:

  "random"    letters drawn from "abcd": many different pairs per word, so several members of one
              batched trip hit the same word
  "runs"      runs of "a" and "b" in turn, run lengths from {1, 2, 3, 4, 5, 7, 8, the rest of the
              word}: a == b merges, odd and even runs, non-overlapping left-to-right matches
  "periodic"  a short period ("ab", "abc", "aab", "abcd", "abcab") repeated from a random phase:
              one pair occurs dozens of times in one word

to_exhaustion(kind, seed) is the text for the runs that go on until no pair is left: for "random"
one word at each length from 1000 on, so that the device's serial scan of a shrinking 4 KB word
takes 2 s and not 6.  single_length_case(L): three words of pre-token length L and nothing
else (one slot class, or only the long table, is occupied).  many_long_case(): more long words
than the long-word blocks have threads.  replay_classes() follows the oracle's merges over the distinct words in plain
Python and counts the rewrites per class, so a test can assert on the CPU that the texts still
reach every class (tests/test_word_length_cases.py).

The generator is the integer-only SplitMix64 of tests/golden/synth_text.py: the texts are the
same on every machine and Python version.
"""
from __future__ import annotations

from synth_text import SplitMix64

KINDS = ("random", "runs", "periodic")
SEEDS = (0, 1, 2)
# pre-token byte lengths, leading space included: both sides of 7|8, 15|16, 31|32 and 63|64, and
# long words up to one of more than 4096 bytes
LENGTHS = (2, 3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 66, 128, 129, 256, 257, 1000, 4097)
REPEATS = (1, 2, 3, 5, 40)
WORDS_PER_LENGTH = 3
VOCABS = (300, 1500, 66000)   # no compaction inside the loop; two; the u32 ids, to exhaustion

_RUN_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 0)   # 0: the rest of the word
_PERIODS = ("ab", "abc", "aab", "abcd", "abcab")
_KIND_SALT = {"random": 1, "runs": 2, "periodic": 3}

MANY_LONG_WORDS = 16640       # > 64 blocks * 256 threads = 16384: the long-word stride loop runs
MANY_LONG_VOCAB = 2000


def _letters(r: SplitMix64, kind: str, n: int) -> str:
    if kind == "random":
        return "".join("abcd"[r.below(4)] for _ in range(n))
    if kind == "runs":
        out, have, which = [], 0, r.below(2)
        while have < n:
            k = _RUN_LENGTHS[r.below(len(_RUN_LENGTHS))]
            k = n - have if k == 0 else min(k, n - have)
            out.append("ab"[which] * k)
            have += k
            which ^= 1
        return "".join(out)
    if kind == "periodic":
        p = _PERIODS[r.below(len(_PERIODS))]
        phase = r.below(len(p))
        return (p * ((n + phase) // len(p) + 1))[phase:phase + n]
    raise ValueError(kind)


def _distinct_words(r: SplitMix64, kind: str, n_letters: int, want: int):
    words: list = []
    for _ in range(64 * want):     # (a kind may have fewer than `want` words of this length)
        w = _letters(r, kind, n_letters)
        if w not in words:
            words.append(w)
            if len(words) == want:
                break
    return words


def _shuffle(r: SplitMix64, items: list):
    for i in range(len(items) - 1, 0, -1):
        j = r.below(i + 1)
        items[i], items[j] = items[j], items[i]


def _join(words) -> str:
    return "".join(" " + w for w in words)   # every pre-token is " " + word


def case(kind: str, seed: int, long_words: int = WORDS_PER_LENGTH) -> str:
    """long_words: the distinct words at the lengths from 1000 on (see to_exhaustion)."""
    r = SplitMix64(seed * 0x100000001B3 + 0x5157 * _KIND_SALT[kind])
    out = []
    for L in LENGTHS:
        reps = list(REPEATS)    # the words of one length draw different counts: at most one has 40,
        _shuffle(r, reps)       # so a text is at most 48 * sum(LENGTHS) = 302 496 bytes
        if L == LENGTHS[-1]:    # the longest always has it: its pairs outnumber the others', and
            reps.sort(reverse=True)   # the merges build it up into tokens of thousands of bytes
        words = _distinct_words(r, kind, L - 1, WORDS_PER_LENGTH)
        for w, k in zip(words[:long_words] if L >= 1000 else words, reps):
            out.extend([w] * k)
    _shuffle(r, out)
    return _join(out)


def to_exhaustion(kind: str, seed: int) -> str:
    """The text for a run until no pair is left (vocab 66 000).  A word of n random letters takes
    about n rounds of its own to become one token, and in each of them the device scans what is
    left of it serially (rewrite_word, one thread per long word): about n * n / 2 id reads in a
    row, measured at 2 s for n = 4096 on an MI355X.  So "random" keeps one word at each length
    from 1000 on there (same letters, same counts, as the first of case()'s three); "runs" and
    "periodic" run out of pairs within 900 rounds and stay whole."""
    return case(kind, seed, 1 if kind == "random" else WORDS_PER_LENGTH)


def all_cases():
    return [(kind, seed) for kind in KINDS for seed in SEEDS]


def single_length_case(L: int) -> str:
    r = SplitMix64(0x51E0000 + L)
    w = _distinct_words(r, "random", L - 1, WORDS_PER_LENGTH)
    return _join([w[0], w[1], w[0], w[2], w[0]])


def many_long_case(n_words: int = MANY_LONG_WORDS) -> str:
    """n_words distinct words of 64-72 letters over "abcdefgh" (pre-tokens of 65-73 bytes)."""
    r = SplitMix64(0x10A6)
    seen, out = set(), []
    while len(out) < n_words:
        w = "".join("abcdefgh"[r.below(8)] for _ in range(64 + r.below(9)))
        if w not in seen:
            seen.add(w)
            out.append(w)
    return _join(out)


def class_of(n_ids: int) -> int:
    """The slot class of a word of n_ids ids (csrc/train.hip class_for); 4: the long table."""
    return 0 if n_ids <= 7 else 1 if n_ids <= 15 else 2 if n_ids <= 31 else 3 if n_ids <= 63 else 4


def replay_classes(words, merges):
    """Apply `merges` in order to each of `words` (bytes) with the reference's rewrite -- every
    non-overlapping occurrence, left to right -- and return a dict:
      rewrites[c]     rewrites of a word that had class c when the merge came
      multi[c]        those with more than one occurrence in the word
      transitions     {(class before, class after): count} over the rewrites that changed it
      to_63           rewrites that took a long word to exactly 63 ids
      single          words that end as one token"""
    ws = [[bytes([b]) for b in w] for w in words]
    rewrites, multi, transitions, to_63 = [0] * 5, [0] * 5, {}, 0
    for a, b in merges:
        new = a + b
        for k, w in enumerate(ws):
            if len(w) < 2 or a not in w or b not in w:
                continue
            out, i, hits, n = [], 0, 0, len(w)
            while i < n:
                if i + 1 < n and w[i] == a and w[i + 1] == b:
                    out.append(new)
                    hits += 1
                    i += 2
                else:
                    out.append(w[i])
                    i += 1
            if not hits:
                continue
            c0, c1 = class_of(n), class_of(len(out))
            rewrites[c0] += 1
            multi[c0] += hits > 1
            if c0 != c1:
                transitions[(c0, c1)] = transitions.get((c0, c1), 0) + 1
            to_63 += c0 == 4 and len(out) == 63
            ws[k] = out
    return {"rewrites": rewrites, "multi": multi, "transitions": transitions, "to_63": to_63,
            "single": sum(len(w) == 1 for w in ws)}
