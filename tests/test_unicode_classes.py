"""CPU: the character classes of the pre-tokenizer over every Unicode scalar value.

The GPT-2 pattern of the reference asks the `regex` module for \\p{L}, \\p{N} and \\s.  Here the two
CPU restatements -- the C oracle (oracle/bpe_oracle.c with the ranges of oracle/uclass_ranges.h)
and the library's host twin of the device's token-start predicate (bpe_pretok_starts_host, with
the paged tables of csrc/uniclass_tables.inc) -- are held against `regex` itself on texts that
contain all 1,112,063 scalar values but U+000D (tests/unicode_cases.py), and both generated
tables are decoded and compared with the installed `regex` code point by code point.  This is
what makes the oracle a reference for tests/test_gpu_unicode.py, where `regex` may be missing.

About 2 s per plane and text on one core, nearly all of it `regex` finditer.
"""
from __future__ import annotations

import collections

import numpy as np
import pytest

regex = pytest.importorskip("regex")

import unicode_cases as U  # noqa: E402
from oracle import cpu_ref  # noqa: E402
from oracle import oracle  # noqa: E402
from test_tokstart import starts_predicate  # noqa: E402


def _byte_offsets(text: str) -> np.ndarray:
    """byte offset of each character of text in its UTF-8 encoding"""
    cp = np.frombuffer(text.encode("utf-32-le", "surrogatepass"), dtype=np.uint32)
    n = 1 + (cp >= 0x80).astype(np.int64) + (cp >= 0x800) + (cp >= 0x10000)
    return np.concatenate(([0], np.cumsum(n)[:-1]))


def check_against_regex(text: str):
    data = text.encode("utf-8")
    off = _byte_offsets(text)
    words = collections.Counter()
    starts = []
    for m in cpu_ref.GPT2_SPLIT.finditer(text):
        starts.append(m.start())
        words[m.group()] += 1
    want = np.zeros(len(data), dtype=np.uint8)
    want[off[np.asarray(starts, dtype=np.int64)]] = 1
    got = starts_predicate(data)
    if not np.array_equal(got, want):
        i = int(np.nonzero(got != want)[0][0])
        ci = int(np.searchsorted(off, i, side="right")) - 1
        pytest.fail(f"token start differs at byte {i} (U+{ord(text[ci]):04X}): host predicate {got[i]}, "
                    f"regex {want[i]}; context {text[max(0, ci - 4):ci + 4]!r}")
    got_words = oracle.word_counts(data, [])
    want_words = {w.encode("utf-8"): c for w, c in words.items()}
    if got_words != want_words:
        diff = sorted(set(got_words.items()) ^ set(want_words.items()), key=lambda kv: (len(kv[0]), kv[0]))
        pytest.fail(f"oracle word counts differ from regex in {len(diff)} entries, e.g. "
                    f"{[(w.decode('utf-8'), c) for w, c in diff[:4]]!r}")


@pytest.mark.parametrize("plane", U.PLANES)
def test_context_text(plane):
    check_against_regex(U.context_text(plane))


@pytest.mark.parametrize("plane", U.PLANES)
def test_class_runs(plane):
    check_against_regex(U.class_run_text(plane))


def test_texts_cover_every_scalar_value():
    seen = set()
    for plane in U.PLANES:
        seen.update(U.context_text(plane))
    seen -= set("a1! 's\n")
    want = {chr(c) for plane in U.PLANES for c in U.scalars(plane)} - set("a1! 's\n")
    assert seen == want
    assert len(want) + len(set("a1! 's\n")) == U.N_SCALARS == 1_112_063
    runs = set()
    for plane in U.PLANES:
        runs.update(U.class_run_text(plane))
    assert runs == want | set("a1! 's\n")


def _regex_classes() -> bytes:
    text = "".join(map(chr, range(0x110000)))   # (lone surrogates included: class other)
    cls = bytearray(0x110000)
    for k, pat in ((U.LETTER, r"\p{L}+"), (U.NUMBER, r"\p{N}+"), (U.SPACE, r"\s+")):
        for m in regex.finditer(pat, text):
            assert not any(cls[m.start():m.end()])   # the three classes are disjoint
            cls[m.start():m.end()] = bytes([k]) * (m.end() - m.start())
    return bytes(cls)


@pytest.mark.parametrize("which", ["device", "oracle"])
def test_generated_tables_match_installed_regex(which):
    """csrc/uniclass_tables.inc (gen_uniclass.py) and oracle/uclass_ranges.h (gen_tables.py) give
    every code point the class the installed `regex` gives it; if not, regenerate both."""
    path, got = ((U.TABLES_INC, U.device_classes()) if which == "device"
                 else (U.RANGES_H, U.oracle_classes()))
    want = _regex_classes()
    if got != want:
        cp = next(i for i in range(0x110000) if got[i] != want[i])
        n = sum(1 for i in range(0x110000) if got[i] != want[i])
        pytest.fail(f"{path.name} (generated with regex {U.generated_with(path)}) differs from the installed "
                    f"regex {regex.__version__} at {n} code points, first U+{cp:04X}: table {got[cp]}, "
                    f"regex {want[cp]} (0 other, 1 L, 2 N, 3 s)")
