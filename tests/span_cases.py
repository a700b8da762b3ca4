"""Encode with offsets: the reference for the spans and the inputs built for their edges.

spans_ref() restates Tokenizer.encode with the structure of oracle/cpu_ref.py's Encoder (reference
models/tokenizer/tokenizer.py:63-138) and keeps what the reference throws away: a running byte
position.  Segments come from the split on the specials, pre-tokens from GPT2_SPLIT.finditer on
each segment, the ids from the merge loop on byte pieces; the span of an id is its final merge
piece's bytes, a special's span the special, and a pre-token equal to a special is dropped with
its bytes (the next span starts past it).  unit "char" maps a byte span by the rule of
include/bpe355.h: C(p) = the non-continuation bytes of data[0:p], start -> C(start) - (1 if
data[start] is a continuation byte), end -> C(end).

The inputs: characters of 2, 3 and 4 bytes at the ends of a 64-byte block and of a 16 KiB chunk,
dropped pre-tokens, specials at every edge, words by id count, batches with seams on the chunk
grid, and the shared-id vocabularies.
"""
from __future__ import annotations

import functools
import random

import regex

import gpt2_files
from oracle.cpu_ref import GPT2_SPLIT, Encoder

K_CHUNK = 16384
K_BLOCK = 64
EOT = "<|endoftext|>"
OVERLAPPING = ["<|endoftext|>", "<|endoftext|><|endoftext|>"]


# ---------------------------------------------------------------------- the reference
class SpanRef:
    """the restatement for one tokenizer; a word's pieces are computed once (they depend on its
    bytes alone, tokenizer.py:124-136)"""

    def __init__(self, vocab, merges, specials):
        self.enc = Encoder(vocab, merges, specials)
        self.inv_merges = {pair: i for i, pair in enumerate(self.enc.merges)}
        self.pieces_of: dict = {}

    def pieces(self, b: bytes):
        raw = self.pieces_of.get(b)
        if raw is None:
            inf = float("inf")
            raw = [bytes([x]) for x in b]
            while len(raw) > 1:
                pair = min(zip(raw, raw[1:]), key=lambda q: self.inv_merges.get(q, inf))
                if pair not in self.inv_merges:
                    break
                raw = Encoder.merge(raw, pair, pair[0] + pair[1])
            self.pieces_of[b] = raw
        return raw

    def byte_spans(self, text, pretokens=None):
        """(ids, byte spans) of one document; `pretokens` replaces GPT2_SPLIT.finditer's matches of
        every non-special segment (a test hands it a pre-token equal to a special)"""
        enc = self.enc
        ids, spans = [], []
        pos = 0   # bytes of the text before the current segment
        segments = regex.split(enc.segment_rgx, text) if enc.segment_rgx else [text]
        for seg in segments:
            if seg == "":
                continue
            seg_bytes = len(seg.encode("utf-8"))
            if seg in enc.special_tokens:
                ids.append(enc.vocab_inv[seg.encode("utf-8")])
                spans.append((pos, pos + seg_bytes))
                pos += seg_bytes
                continue
            p = pos
            for s in (pretokens(seg) if pretokens else (m.group(0) for m in GPT2_SPLIT.finditer(seg))):
                b = s.encode("utf-8")
                if s in enc.special_tokens:   # dropped (tokenizer.py:73): bytes without an id
                    p += len(b)
                    continue
                for piece in self.pieces(b):
                    ids.append(enc.vocab_inv[piece])
                    spans.append((p, p + len(piece)))
                    p += len(piece)
            assert p == pos + seg_bytes, "the pre-tokens tile their segment"
            pos += seg_bytes
        return ids, spans

    def spans(self, text, unit="char"):
        ids, spans = self.byte_spans(text)
        if unit == "byte":
            return ids, spans
        if unit != "char":
            raise ValueError("unit is 'byte' or 'char'")
        return ids, to_chars(text.encode("utf-8"), spans)


def byte_spans_ref(vocab, merges, specials, text):
    """(ids, byte spans) of one document"""
    return SpanRef(vocab, merges, specials).byte_spans(text)


def char_index(data: bytes, p: int) -> int:
    """C(p): the bytes of data[0:p] that are not continuation bytes"""
    return sum((b & 0xC0) != 0x80 for b in data[:p])


def to_chars(data: bytes, spans):
    pre = [0]
    for b in data:
        pre.append(pre[-1] + ((b & 0xC0) != 0x80))
    return [(pre[s] - (1 if (data[s] & 0xC0) == 0x80 else 0), pre[e]) for s, e in spans]


def spans_ref(vocab, merges, specials, text, unit="char"):
    """(ids, spans) of encode(text), the spans in bytes of text.encode() or in characters of text"""
    return SpanRef(vocab, merges, specials).spans(text, unit)


# ---------------------------------------------------------------------- tokenizers
@functools.lru_cache(maxsize=None)
def gpt2(specials=()):
    return gpt2_files.load_gpt2(list(specials))


@functools.lru_cache(maxsize=None)
def small():
    """the reference's trained vocab of 500: non-ASCII characters split across tokens"""
    return gpt2_files.load_reference_train_golden()


def fixture_text(name: str) -> str:
    return (gpt2_files.FIXTURES / name).read_text(encoding="utf-8")


# A vocab dict maps each id to one byte string, so two byte strings reach one id only through the
# reference's bookkeeping for a special that the vocab lacks (tokenizer.py:35-38): it gets the id
# len(vocab), which a vocab with a gap in its ids may have given to another entry already.
def shared_len_vocab():
    """(vocab, merges, specials): the missing special takes id 256, which b"\xff" holds -- one id,
    byte strings of 13 bytes and of 1 byte: the span calls refuse this tokenizer"""
    v = {i: bytes([i]) for i in range(255)}
    v[256] = b"\xff"
    return v, [], [EOT]


def shared_same_len_vocab():
    """(vocab, merges, specials): the missing special "Z" takes id 255, which b"\xff" holds -- one
    id, two byte strings of one byte: every id still has one length and the spans are exact"""
    v = {i: bytes([i]) for i in range(256) if i != ord("Z")}
    return v, [], ["Z"]


# ---------------------------------------------------------------------- character edges
CHARS = {2: "é", 3: "€", 4: "😀"}     # by UTF-8 length


def char_edge_texts(boundary: int):
    """texts in which a character of 2, 3 and 4 bytes begins at boundary + d for d in -4 .. 4, after
    ASCII filler: the character's bytes straddle the boundary for the negative d that reach it.
    Under the small vocab its bytes fall into different tokens."""
    out = []
    for nb, ch in CHARS.items():
        for d in range(-4, 5):
            at = boundary + d
            fill = ("word " * (at // 5 + 1))[:at]
            text = fill + ch + " tail" + ch * 2 + " end"
            assert len(fill.encode()) == at
            out.append((f"{nb}B@{boundary}{d:+d}", text))
    return out


def char_edge_batches(boundary: int):
    """a document that starts right after a character ending at boundary + d"""
    out = []
    for nb, ch in CHARS.items():
        for d in (-1, 0, 1):
            end = boundary + d
            at = end - nb
            first = ("word " * (at // 5 + 1))[:at] + ch
            out.append((f"doc-after-{nb}B@{boundary}{d:+d}", [first, ch + "next" + ch, "", "x" + ch]))
    return out


# ---------------------------------------------------------------------- dropped pre-tokens, specials
# A pre-token equal to a special is dropped by the reference (tokenizer.py:73) and k_encode_words
# gives it the info 0, so the spans would show a gap there.  It cannot be reached through encode():
# the split on the specials tries every special at every position that no earlier match covers,
# so a segment that is not a special holds no occurrence of one, and a pre-token is a substring of
# its segment.  find_drop() searches for a counter-example (every text over a small alphabet up to
# max_len characters, every pair of candidate specials); tests/test_span_cases.py pins that there
# is none, and that the restatement does drop such a pre-token when it is handed one.
DROP_ALPHABET = ["a", " ", "'", "s", "!"]
DROP_SPECIALS = ["'s", " a", "a", "!", " !", "s", " ", "  ", "a'", "!!", " a'", "as"]


def find_drop(max_len=4):
    """(specials, text) whose pre-tokenization yields a pre-token equal to a special, or None"""
    import itertools
    for n in range(1, max_len + 1):
        for t in itertools.product(DROP_ALPHABET, repeat=n):
            text = "".join(t)
            for sp in itertools.combinations(DROP_SPECIALS, 2):
                rgx = "(" + "|".join(regex.escape(x) for x in sorted(sp, key=len, reverse=True)) + ")"
                for seg in regex.split(rgx, text):
                    if seg == "" or seg in sp:
                        continue
                    if any(m.group(0) in sp for m in GPT2_SPLIT.finditer(seg)):
                        return list(sp), text
    return None


def special_texts():
    """(name, specials, text): specials adjacent, at byte 0, at the end, missing from the vocab,
    overlapping (longest first)"""
    e = EOT
    return [
        ("adjacent", [e], f"{e}{e}{e}"),
        ("at-0-and-end", [e], f"{e}hello world{e}"),
        ("between", [e], f"héllo{e} wörld {e}{e} x"),
        ("missing", ["<|missing|>", e], f"a<|missing|>b{e}<|missing|>"),
        ("overlapping", OVERLAPPING, f"a{e}{e}{e} b{e}"),
        ("only", [e], e),
    ]


# ---------------------------------------------------------------------- words by id count
def id_count_words():
    """words of the emit-case tokenizer (tests/emit_cases.py) with 1, 2, 3, 4, 5 and more ids: the
    inline infos and the pool; vocab entries of several ids come from the dictionary pool"""
    import emit_cases as ec
    words = [" ab", " x", " xy", " xyz", " xyzx", " xyzxy", " xyzxyzxyz", " " + ec.GH16, " " + ec.JK15,
             " abx", " ababab", "jkjkx", " " + "xyz" * 7, " " + "zyx" * 20]
    rnd = random.Random(7)
    text = "".join(rnd.choice(words) for _ in range(4000))
    return text


# ---------------------------------------------------------------------- batches
def seam_batches():
    """documents whose seams lie on and next to chunk boundaries, empty documents first, last and in
    a row, one document"""
    base = fixture_text("corpus.en")
    body = base.encode("ascii", "ignore").decode()[: 3 * K_CHUNK]   # ASCII: a character is a byte
    out = [("one", [body[:5000]]), ("empties", ["", "", "abc", "", "", "déf", ""]), ("all-empty", ["", "", ""])]
    for d in (-2, -1, 0, 1, 2):
        a = K_CHUNK + d
        b = 2 * K_CHUNK - d
        out.append((f"seam{d:+d}", ["", body[:a], body[a:b], "", body[b:], ""]))
    return out


def sliced_batch(n_docs=3000, seed=11):
    """a few thousand seeded slices of corpus.en"""
    base = fixture_text("corpus.en")
    rnd = random.Random(seed)
    docs = []
    for _ in range(n_docs):
        a = rnd.randrange(len(base) - 400)
        docs.append(base[a:a + rnd.randrange(0, 300)])
    return docs


SHORT_TEXTS = ["", "a", "é", "ab", "héllo wörld😀"]     # 0, 1, 2, 2 and 17 bytes
