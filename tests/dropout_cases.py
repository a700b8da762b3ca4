"""Encode with BPE-dropout: the reference and the inputs built for the device path's edges.

DropoutRef restates the semantics of include/bpe355.h (bpe_tok_encode_dropout) on top of
oracle/cpu_ref.py's Encoder.  Segmentation on the specials, the GPT-2 pre-tokenization, the dropping
of a pre-token equal to a special and the id lookup (KeyError) are Encoder's; a special yields its
one id and draws nothing.  Only the merge loop of a pre-token changes:

    M64 = 2**64 - 1
    mix64(z): z ^= z >> 30; z = z * 0xBF58476D1CE4E5B9 & M64; z ^= z >> 27;
              z = z * 0x94D049BB133111EB & M64; return z ^ (z >> 31)
    thr = int(round(p * 2**24))
    word_key(seed, doc_key, off) = mix64(mix64(mix64((seed + 0x9E3779B97F4A7C15) & M64) ^ doc_key) ^ off)
        off: the byte offset of the pre-token's first byte in its document
    dropped(wk, rnd, pos) = (mix64(wk ^ (rnd << 32 | pos)) >> 40) < thr
        rnd: the round 0, 1, 2, ...; pos: the byte offset, inside the pre-token, of the pair's left token

    rank = {pair: i for i, pair in enumerate(merges)}      # a repeated pair keeps its LAST index
    t = the single bytes of the pre-token, st[j] = the byte offset of t[j], rnd = 0
    while len(t) > 1:
        best = the ranked adjacent pair (t[j], t[j + 1]) of minimum rank among the positions j that
               are not dropped(wk, rnd, st[j]); none: stop (also when ranked pairs remain)
        rewrite left to right: at i, if (t[i], t[i + 1]) == best and not dropped(wk, rnd, st[i]):
               emit t[i] + t[i + 1], i += 2; else emit t[i], i += 1
        rnd += 1

p = 0 is encode() exactly, p = 1 gives every byte its own id, and a document's ids depend on
(seed, doc_key, text) alone.
"""
from __future__ import annotations

import functools
import pathlib
import re

import regex

import emit_cases as ec
import gpt2_files
import span_cases as sc
from oracle.cpu_ref import GPT2_SPLIT, Encoder

M64 = 2 ** 64 - 1
K_CHUNK = 16384
K_BLOCK = 64
EOT = "<|endoftext|>"
ROOT = pathlib.Path(__file__).resolve().parent.parent


def mix64(z: int) -> int:
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & M64
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & M64
    return z ^ (z >> 31)


def thr_of(p) -> int:
    return int(round(p * 2 ** 24))


def word_key(seed: int, doc_key: int, off: int) -> int:
    h = mix64((seed + 0x9E3779B97F4A7C15) & M64)
    h = mix64(h ^ doc_key)
    return mix64(h ^ off)


def draw(wk: int, rnd: int, pos: int) -> int:
    return mix64(wk ^ (rnd << 32 | pos)) >> 40


def draw_of(seed, doc_key, off, rnd, pos) -> int:
    return draw(word_key(seed, doc_key, off), rnd, pos)


class DropoutRef(Encoder):
    """the restatement for one tokenizer; n_draws / n_dropped count the draws of the ranked pairs
    (one per pair and round) since the last reset_stats()"""

    def __init__(self, vocab, merges, specials=None):
        super().__init__(vocab, merges, specials)
        self.rank = {pair: i for i, pair in enumerate(self.merges)}
        self.reset_stats()

    def reset_stats(self):
        self.n_draws = self.n_dropped = 0

    def pretokens_at(self, text: str):
        """(byte offset in the document, pre-token or special, is_special) in order; pre-tokens
        equal to a special are left out (their bytes still count)"""
        out, pos = [], 0
        segments = regex.split(self.segment_rgx, text) if self.segment_rgx else [text]
        for seg in segments:
            if seg == "":
                continue
            if seg in self.special_tokens:
                out.append((pos, seg, True))
                pos += len(seg.encode("utf-8"))
                continue
            for m in GPT2_SPLIT.finditer(seg):
                s = m.group(0)
                if s not in self.special_tokens:
                    out.append((pos, s, False))
                pos += len(s.encode("utf-8"))
        return out

    def merge_word(self, b: bytes, wk: int, thr: int):
        rank = self.rank
        t = [bytes([x]) for x in b]
        st = list(range(len(b)))
        rnd = 0
        while len(t) > 1:
            best, best_pair, live = None, None, []
            for j in range(len(t) - 1):
                r = rank.get((t[j], t[j + 1]))
                if r is None:
                    live.append(False)
                    continue
                d = thr > 0 and draw(wk, rnd, st[j]) < thr
                self.n_draws += 1
                self.n_dropped += d
                live.append(not d)
                if not d and (best is None or r < best):
                    best, best_pair = r, (t[j], t[j + 1])
            if best is None:
                break
            nt, ns, i = [], [], 0
            while i < len(t):
                if i + 1 < len(t) and live[i] and (t[i], t[i + 1]) == best_pair:
                    nt.append(t[i] + t[i + 1])
                    ns.append(st[i])
                    i += 2
                else:
                    nt.append(t[i])
                    ns.append(st[i])
                    i += 1
            t, st = nt, ns
            rnd += 1
        return t

    def encode_dropout(self, text: str, p, seed: int, doc_key: int = 0):
        thr = thr_of(p)
        ids = []
        for off, s, special in self.pretokens_at(text):
            b = s.encode("utf-8")
            if special:
                ids.append(self.vocab_inv[b])
                continue
            ids.extend(self.vocab_inv[x] for x in self.merge_word(b, word_key(seed, doc_key, off), thr))
        return ids

    def encode_batch_dropout(self, texts, p, seed: int, doc_base: int = 0):
        return [self.encode_dropout(t, p, seed, doc_base + i) for i, t in enumerate(texts)]

    def decode(self, ids) -> str:
        by_id = {i: b for b, i in self.vocab_inv.items()}   # (a missing special has an id only here)
        return b"".join(by_id[i] for i in ids).decode("utf-8", errors="replace")


# ---------------------------------------------------------------------- known answers
DRAWS = [   # (seed, doc_key, off, rnd, pos) -> draw
    ((0, 0, 0, 0, 0), 1660839),
    ((7, 0, 0, 0, 0), 5435882),
    ((7, 3, 12, 1, 2), 7754368),
    ((2 ** 64 - 1, 2 ** 40 + 5, 2 ** 32 - 1, 5, 8388607), 3816701),
]
THRS = {0.1: 1677722, 0.5: 8388608, 1.0: 16777216, 0: 0}


def doubling(n: int = 6):
    """(vocab, merges): the 256 bytes and (a, a), (aa, aa), ... n doublings, ids 256, 257, ..."""
    vocab = {i: bytes([i]) for i in range(256)}
    merges = []
    w = b"a"
    for _ in range(n):
        merges.append((w, w))
        w = w + w
        vocab[len(vocab)] = w
    return vocab, merges


AAAA = {   # "aaaa aaaa" under doubling(), p = 0.5: (seed, doc_key) -> ids
    (0, 0): [97, 97, 97, 97, 32, 97, 97, 256],
    (1, 0): [257, 32, 256, 256],
    (3, 0): [256, 256, 32, 257],
    (0, 1): [256, 256, 32, 256, 97, 97],
}


def repeated_pair():
    """(vocab, merges, text, ids at p = 0): (a, b) is listed twice and keeps its LAST index 2, so
    (b, c) at 1 merges first: "abc" -> a, bc (the first index would give ab, c)"""
    vocab = {i: bytes([i]) for i in range(256)}
    vocab[256], vocab[257] = b"ab", b"bc"
    merges = [(b"a", b"b"), (b"b", b"c"), (b"a", b"b")]
    return vocab, merges, "abc abc", [97, 257, 32, 97, 257]


# ---------------------------------------------------------------------- tokenizers, fixtures
gpt2 = sc.gpt2
small = sc.small
fixture_text = sc.fixture_text


def emit_tokenizer():
    """the emit-case tokenizer (tests/emit_cases.py): (vocab, merges, specials)"""
    return ec.vocab(), ec.merges(), [EOT]


def stats_text() -> str:
    c = fixture_text("corpus.en")
    return c[:20000] + EOT + c[20000:60000]


FIXTURE_TEXTS = {
    "address": lambda: fixture_text("address.txt"),
    "german": lambda: fixture_text("german.txt"),
    "corpus40k": lambda: fixture_text("corpus.en")[:40000],
    "tiny40k": lambda: fixture_text("tinystories_sample.txt")[:40000],
}


def with_specials(text: str, kind: str):
    """(specials, text) for kind "none", "eot" (one EOT mid-text and one at the end) and "overlap"
    (span_cases.OVERLAPPING: runs of two and three EOTs)"""
    h = len(text) // 2
    if kind == "none":
        return [], text
    if kind == "eot":
        return [EOT], text[:h] + EOT + text[h:] + EOT
    assert kind == "overlap"
    return list(sc.OVERLAPPING), text[:h] + EOT * 3 + text[h:] + EOT * 2 + " x" + EOT


# ---------------------------------------------------------------------- the device path's bounds
@functools.lru_cache(maxsize=None)
def short_bound() -> int:
    """kDropShort of csrc/dropout.hip: the longest pre-token of the one-lane path"""
    src = (ROOT / "transformer-lm_amd" / "csrc" / "dropout.hip").read_text()
    return int(re.search(r"constexpr int kDropShort = (\d+);", src).group(1))


CHARS = sc.CHARS   # by UTF-8 length: é (a letter), € and 😀 (neither letter nor number)


def one_word(n_bytes: int, lead: bool, ch: str | None):
    """a single pre-token of exactly n_bytes bytes: an optional leading space, then the filler
    with `ch` at both ends (once when only one fits); the filler is of ch's class, so the GPT-2
    pattern keeps the word whole.  None when n_bytes is too small for the form."""
    fill = "a" if ch in (None, "é") else "#"
    body = n_bytes - (1 if lead else 0)
    if ch is None:
        return (" " if lead else "") + fill * body if body >= 1 else None
    cb = len(ch.encode("utf-8"))
    if body >= 2 * cb:
        w = ch + fill * (body - 2 * cb) + ch
    elif body >= cb + 1 or body == cb:
        w = ch + fill * (body - cb)
    else:
        return None
    return (" " if lead else "") + w


def word_lengths():
    k = short_bound()
    return [1, 2, 3, k - 1, k, k + 1, 64, 65, 256]


def word_length_docs():
    """[(n_bytes, word)]: every form of one_word at every length of word_lengths(); each word is a
    document of its own, so it is one pre-token at offset 0"""
    out = []
    for n in word_lengths():
        for lead in (False, True):
            for ch in (None, "é", "€", "😀"):
                w = one_word(n, lead, ch)
                if w is not None:
                    out.append((n, w))
    return out


LONG_AS = (4097, 40960)   # "a" * n under doubling(): overlapping occurrences, many rounds, the long path


def edge_texts(boundary: int):
    """[(name, text, (start, end))]: a short and a long word (2 and short_bound() + 9 bytes past the
    space) that ends at, starts at and straddles `boundary`, in ordinary short words of the emit-case
    tokenizer; (start, end) are the word's bytes"""
    out = []
    for wname, w in (("short", " ababxab"), ("long", " " + "abxgh" * ((short_bound() + 9) // 5 + 1))):
        n = len(w)
        for mode, start in (("ends-at", boundary - n), ("starts-at", boundary), ("straddles", boundary - n // 2)):
            t = ec._Text()
            t.fill_to(start)
            t.add(w)
            t.add(" tail ab xyz")
            out.append((f"{wname}-{mode}-{boundary}", t.text(), (start, start + n)))
    return out
