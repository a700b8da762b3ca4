"""Training inputs whose tied pairs are ordered past the 8-byte prefix key.

The trainer picks max over (count, bytes a, bytes b) (reference train.py:187-189).  The device
compares tokens by a zero-padded 8-byte prefix first (csrc/train.hip cand_better) and looks at
the bytes themselves (cmp_tok_tail: bytes from index 8 on, then the length) only when two
different tokens have equal padded prefixes.  These texts make that the deciding comparison:

  "prefix"   words "abababab" + a tail over "ab": tokens grow past 8 bytes with equal prefixes
  "nul"      words over "\\x00\\x01": "\\x00" against "\\x00\\x00" pad to the same key
  "nulstem"  words "\\x00" * 8 + a tail over "\\x00\\x01": both at once, one word per line

deep_rounds() counts, with oracle/cpu_ref.py alone, the rounds in which the winner and the best
tied runner-up were told apart that way, so a test can assert that it still reaches the case.
"""
from __future__ import annotations

import random

KINDS = ("prefix", "nul", "nulstem")
SEEDS = (0, 1, 2, 3)
VOCAB = 406            # 150 merges, no specials
SCALED_WORDS = 2000
SCALED_VOCAB = 1200

_SPEC = {   # kind: stem, tail alphabet, tail length lo..hi, separator
    "prefix": ("abababab", "ab", 1, 16, " "),
    "nul": ("", "\x00\x01", 2, 20, " "),
    "nulstem": ("\x00" * 8, "\x00\x01", 1, 12, "\n"),
}


def case(seed: int, kind: str, n_words: int = 30) -> str:
    stem, alpha, lo, hi, sep = _SPEC[kind]
    r = random.Random(seed)
    words = []
    for _ in range(n_words):
        words.append(stem + "".join(r.choice(alpha) for _ in range(r.randint(lo, hi))))
    reps = r.choice([1, 2, 3])
    words = [w for w in words for _ in range(reps)]
    r.shuffle(words)
    return sep.join(words)


def all_cases():
    return [(kind, seed) for kind in KINDS for seed in SEEDS]


def _pad8(b: bytes) -> bytes:
    return b[:8].ljust(8, b"\0")


def deep_rounds(text: str, vocab_size: int, specials=()):
    """(rounds decided by a byte at index >= 8, rounds decided by length): rounds of
    cpu_ref.train in which the winner's count is tied and the deciding parts (the first parts if
    they differ, else the second parts) of the winner and of the best tied runner-up have equal
    zero-padded 8-byte prefixes."""
    from oracle import cpu_ref
    by_byte = by_len = 0

    def on_round(pairs, best):
        nonlocal by_byte, by_len
        c = pairs[best]
        tied = [p for p, n in pairs.items() if n == c and p != best]
        if not tied:
            return
        second = max(tied)
        x, y = (best[0], second[0]) if best[0] != second[0] else (best[1], second[1])
        if _pad8(x) != _pad8(y):
            return
        m = min(len(x), len(y))
        if x[:m] != y[:m]:
            by_byte += 1     # equal padded prefixes: the first difference is at index >= 8
        else:
            by_len += 1      # one is a prefix of the other
    cpu_ref.train(text, vocab_size, specials, on_round=on_round)
    return by_byte, by_len
