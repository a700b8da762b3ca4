"""Texts that put every Unicode scalar value in front of the pre-tokenizer, and an all-byte-pairs
tokenizer that makes every pre-token boundary next to an ASCII byte visible in the encoded ids.

The pre-tokenizer's classes are \\p{L}, \\p{N}, \\s and other, as the `regex` module defines them
for the GPT-2 pattern.  The generators here need no `regex`: where a text is built by class, the
classes are read from oracle/uclass_ranges.h (tests/test_unicode_classes.py pins that file, and
the device's csrc/uniclass_tables.inc, to the installed `regex` code point by code point).

U+000D is left out everywhere: the text-mode read turns it into U+000A before the
pre-tokenizer sees it.  Surrogates are no scalar values.
"""
from __future__ import annotations

import functools
import pathlib
import re

ROOT = pathlib.Path(__file__).resolve().parent.parent
RANGES_H = ROOT / "oracle" / "uclass_ranges.h"
TABLES_INC = ROOT / "transformer-lm_amd" / "csrc" / "uniclass_tables.inc"

PLANES = range(17)
N_SCALARS = 0x110000 - 0x800 - 1      # no surrogates, no U+000D
OTHER, LETTER, NUMBER, SPACE = 0, 1, 2, 3
K_CHUNK = 16384                       # csrc: kChunk, the bytes one workgroup pre-tokenizes
K_HALO = 1024                         # the staged halo past a chunk


def scalars(plane: int):
    lo = plane << 16
    return [c for c in range(lo, lo + 0x10000) if not (0xD800 <= c <= 0xDFFF) and c != 0x0D]


@functools.lru_cache(maxsize=2)
def context_text(plane: int) -> str:
    """each scalar value of the plane between letters, between digits, between punctuation, and
    doubled in front of a contraction"""
    return "".join(f"a{ch}a 1{ch}1 !{ch}! {ch}{ch}'s\n" for ch in map(chr, scalars(plane)))


# ------------------------------------------------------------------ the generated tables
def _c_array(text: str, name: str):
    m = re.search(name + r"\s*(?:\[[^\]]*\])+\s*=\s*\{(.*?)\};", text, re.S)
    assert m, f"{name} not found"
    return [int(x, 0) for x in re.findall(r"0[xX][0-9A-Fa-f]+|\d+", m.group(1))]


def generated_with(path) -> str:
    """the `regex` version a generated table file records in its header"""
    m = re.search(r"regex`? (\d[\w.]*\d)", pathlib.Path(path).read_text()[:600])
    return m.group(1) if m else "unknown"


@functools.lru_cache(maxsize=None)
def oracle_classes() -> bytes:
    """class of each of the 0x110000 code points by the ranges of oracle/uclass_ranges.h
    (the oracle asks S, L, N in that order; the classes are disjoint)"""
    text = RANGES_H.read_text()
    cls = bytearray(0x110000)
    for name, k in (("ORACLE_N", NUMBER), ("ORACLE_L", LETTER), ("ORACLE_S", SPACE)):
        v = _c_array(text, name)
        for lo, hi in zip(v[0::2], v[1::2]):
            cls[lo:hi + 1] = bytes([k]) * (hi - lo + 1)
    return bytes(cls)


def device_classes() -> bytes:
    """class of each code point as the device reads csrc/uniclass_tables.inc: the ASCII table
    below 128, else 2 bits of the page BPE_UC_PAGE[cp >> 8] (csrc/tokstart.h uc_class)"""
    text = TABLES_INC.read_text()
    ascii_cls = _c_array(text, "BPE_ASCII_CLASS")
    page = _c_array(text, "BPE_UC_PAGE")
    bits = _c_array(text, "BPE_UC_BITS")
    assert len(ascii_cls) == 128 and len(page) == 0x1100 and len(bits) % 64 == 0
    assert max(page) < len(bits) // 64
    cls = bytearray(0x110000)
    for cp in range(0x110000):
        if cp < 128:
            cls[cp] = ascii_cls[cp]
        else:
            cls[cp] = (bits[page[cp >> 8] * 64 + ((cp & 255) >> 2)] >> ((cp & 3) * 2)) & 3
    return bytes(cls)


# ------------------------------------------------------------------ one run per class
def class_members(plane: int, k: int):
    cls = oracle_classes()
    return [c for c in scalars(plane) if cls[c] == k]


@functools.lru_cache(maxsize=2)
def class_run_text(plane: int) -> str:
    """all letters of the plane in code-point order as one run, all numbers, all others, joined
    by one U+0020; then the white space between two ASCII letters.  Each run is one pre-token (up
    to 262 KB), far longer than the staged halo."""
    runs = ["".join(map(chr, class_members(plane, k))) for k in (LETTER, NUMBER, OTHER)]
    text = " ".join(r for r in runs if r)
    ws = "".join(map(chr, class_members(plane, SPACE)))
    if ws:
        text += " a" + ws + "a"
    return text


def serial_scanner_text(run_bytes: int = K_CHUNK):
    """plane 0's letters, numbers and others in code-point order, cut into runs of about
    `run_bytes` bytes (more than the halo) with one U+0020 between runs, which belongs to the
    next run's pre-token.  Each run starts in the chunk where the previous one ends and runs past
    that chunk's end (short " x" filler moves a run that would not), so every run is the last
    pre-token that starts in its chunk: the one whose end the serial scanner finds, past the
    staged halo.  -> (text, [(byte offset, byte length) of each run's pre-token])"""
    assert run_bytes > 2 * K_HALO
    pad = {LETTER: "a", NUMBER: "1", OTHER: "!"}
    out, spans, pos = [], [], 0
    for k in (LETTER, NUMBER, OTHER):
        cur, cur_n, pieces = [], 0, []
        for ch in map(chr, class_members(0, k)):
            cur.append(ch)
            cur_n += len(ch.encode("utf-8"))
            if cur_n >= run_bytes:
                pieces.append(("".join(cur), cur_n))
                cur, cur_n = [], 0
        if cur_n > 2 * K_HALO + 2 or not pieces:   # (a shorter rest joins the run before it)
            pieces.append(("".join(cur), cur_n))
        else:
            pieces[-1] = (pieces[-1][0] + "".join(cur), pieces[-1][1] + cur_n)
        for run, n in pieces:
            tok = n + (1 if pos else 0)
            boundary = (pos // K_CHUNK + 1) * K_CHUNK
            if pos + tok < boundary + K_HALO:   # would end inside its chunk's staged window
                gap = max(0, boundary - tok // 2 - pos) // 2 * 2
                out.append(" x" * (gap // 2))
                pos += gap
                tok = n + (1 if pos else 0)
            start = pos
            out.append((" " if pos else "") + run)
            pos += tok
            if pos % K_CHUNK == 0:   # the next run must start in the chunk where this one ends
                out.append(pad[k])
                pos += 1
            assert pos - 1 >= (start // K_CHUNK + 1) * K_CHUNK
            spans.append((start, pos - start))
    return "".join(out), spans


# ------------------------------------------------------------------ all-byte-pairs tokenizer
@functools.lru_cache(maxsize=None)
def all_pairs_tokenizer():
    """(vocab, merges): the 256 byte tokens and one merge per byte pair, ranked (ASCII,
    non-ASCII), (non-ASCII, ASCII), (ASCII, ASCII), (non-ASCII, non-ASCII): an ASCII byte next
    to a character merges with it if and only if no pre-token boundary lies between them."""
    A, H = range(128), range(128, 256)
    merges = [(bytes([a]), bytes([b])) for xs, ys in ((A, H), (H, A), (A, A), (H, H))
              for a in xs for b in ys]
    vocab = {i: bytes([i]) for i in range(256)}
    for a, b in merges:
        vocab[len(vocab)] = a + b
    assert len(vocab) == 65792
    return vocab, merges
