"""CPU: the big-count training inputs (tests/big_count_cases.py) are what they claim, and their
reference, train_counts, is the reference trainer: it equals the C oracle (itself pinned to the
reference's goldens) on texts' own counts, with and without special tokens, and on every scaled
case it gives the unscaled text's merges.  Everything here comes from the oracle and plain
Python, nothing from the code under test.

Counted at VOCAB = 1200: "synth" has 6136 words and 944 rounds whose best count falls from 3182
to 6; crossing() (times 2^25) has 147 rounds at 2^32 or above, 124 in [2^31, 2^32) and 673 below
2^31 (one shift less leaves fewer than 100 in the first two).  mixed_magnitudes() has 882 rounds at
2^32 or above; its first, (s, t), sums 582 words below 2^32 that alone come to 2.8e11.  The floors
(100 rounds per regime, 100 words) were set before these were counted.
"""
import functools

import pytest

import big_count_cases as B
import golden_cases as G
import tie_cases
from oracle import oracle

EOT = "<|endoftext|>"


@functools.lru_cache(maxsize=None)
def _oracle(text_case, vocab=B.VOCAB):
    return oracle.train_raw(B.text_bytes(text_case), vocab, [])


def _small_texts():
    return {"corpus.en": G.input_bytes({"kind": "fixture", "name": "corpus.en"})[:60_000],
            "synth": B.text_bytes("synth")[:40_000],
            "prefix": tie_cases.case(1, "prefix").encode("utf-8"),
            "nul": tie_cases.case(1, "nul").encode("utf-8"),
            "nulstem": tie_cases.case(1, "nulstem").encode("utf-8")}


@pytest.mark.parametrize("specials", [[], [EOT], [" the", EOT, " ab"]], ids=["none", "eot", "word"])
@pytest.mark.parametrize("name", list(_small_texts()))
def test_train_counts_equals_the_oracle(name, specials):
    """(" the" and " ab" are words of the texts: as specials they leave the counts)"""
    data = _small_texts()[name]
    vocab = tie_cases.VOCAB if name in tie_cases.KINDS else 600
    text = oracle.decode_text(data)
    all_words = oracle.word_counts(text, [])
    counts = oracle.word_counts(text, specials)
    if name == "corpus.en" and " the" in specials:
        assert b" the" in all_words and b" the" not in counts
    want = oracle.train_raw(data, vocab, specials)
    assert B.train_counts(counts, vocab, specials) == want
    assert B.train_counts(all_words, vocab, specials) == want   # train_counts drops the word itself


@pytest.mark.parametrize("k", B.FACTORS)
@pytest.mark.parametrize("text_case", B.TEXT_CASES)
def test_scaled_cases_train_like_the_unscaled_text(text_case, k):
    counts = B.scaled(text_case, k)
    base = B.base_counts(text_case)
    assert counts.keys() == base.keys() and all(counts[w] == k * c for w, c in base.items())
    assert min(counts.values()) >= 1 << 32
    assert B.weight(counts) < B.WEIGHT_LIMIT
    vocab, merges, tops = B.tops(counts, B.VOCAB)
    assert (vocab, merges) == _oracle(text_case)
    assert len(merges) >= 100 and all(t % k == 0 for t in tops)
    if text_case in tie_cases.KINDS:
        # the text and vocab size of test_tie_cases.py's test_scaled_cases_reach_the_deep_comparison,
        # which counts the rounds decided past the 8-byte prefix; here: rounds tied at the top
        assert (tie_cases.SCALED_WORDS, tie_cases.SCALED_VOCAB) == (2000, B.VOCAB)
        assert sum(x == y for x, y in zip(tops, tops[1:])) >= 100


def test_parity_cases_specials():
    """One scaled "synth" case has a special token that is one of its words: the word leaves the
    counts, and the merges change."""
    cases = B.parity_cases()
    word = B.common_word()
    assert [sp for _f, _v, sp in cases.values() if sp] == [(EOT,), (EOT, word)]
    build, vocab, specials = cases[f"scaled-synth-{B.FACTORS[2]:#x}"]
    counts = build()
    assert specials == (EOT, word) and counts[word.encode()] >= 1000 * B.FACTORS[2]
    got = B.train_counts(counts, vocab, specials)
    assert got == oracle.train_raw(B.text_bytes("synth"), vocab, list(specials))
    assert got[1] != _oracle("synth")[1] and got[0][1] == word.encode()
    assert len(cases) == len(B.TEXT_CASES) * 3 + 2 + 2 * len(B.BOUNDARY_VS) + 1


def test_crossing_has_100_rounds_in_each_regime():
    vocab, merges, tops = B.tops(B.crossing(), B.VOCAB)
    assert (vocab, merges) == _oracle("synth")
    high = sum(t >= 1 << 32 for t in tops)
    mid = sum(1 << 31 <= t < 1 << 32 for t in tops)
    low = sum(t < 1 << 31 for t in tops)
    print(f"crossing: {len(tops)} rounds, best count {tops[0]} .. {tops[-1]}: {high} rounds >= 2^32, "
          f"{mid} in [2^31, 2^32), {low} below 2^31")
    assert high >= 100 and mid >= 100 and low >= 100
    assert tops == sorted(tops, reverse=True)    # it falls through 2^32 once, part-way
    assert max(B.crossing().values()) >= 1 << 32   # single words at 2^32 and above, too


def test_grows_pair_table():
    vocab, merges, tops = B.tops(B.grows_pair_table(), B.GROW_VOCAB)
    assert (vocab, merges) == oracle.train_raw(B.text_bytes("nul"), B.GROW_VOCAB, [])
    assert len(merges) == B.GROW_VOCAB - 256
    assert 256 + len(merges) > 2032 + 100       # tokens: 4 * 16 * (tokens + 16) passes 2^18 / 2
    assert tops[-1] >= 1 << 32                  # every live count is still a multiple of 2^33 - 1
    assert all(t % ((1 << 33) - 1) == 0 for t in tops)
    assert all(t >= 1 << 32 for t in tops[2033 - 256:])   # the rounds after the table must have grown


@pytest.mark.parametrize("V", B.BOUNDARY_VS)
def test_boundary(V):
    counts = B.boundary(V)
    assert sum(counts.values()) == V and len(counts) == B.BOUNDARY_WORDS
    assert all(w.startswith(b" xab") for w in counts)
    assert {len(w) - 4 for w in counts} == set(B.BOUNDARY_SUFFIXES)
    assert {B.class_of(len(w)) for w in counts} == {0, 1, 2, 3, 4}
    assert max(counts.values()) <= V // 100
    assert B.weight(counts) < B.WEIGHT_LIMIT
    if V == B.BOUNDARY_VS[-1]:
        assert 1 << 59 <= B.weight(counts) < 1 << 60      # a weight of 60 bits
    _vocab, merges, tops = B.tops(counts, B.BOUNDARY_VOCAB)
    assert merges[:3] == [(b"x", b"a"), (b"xa", b"b"), (b" ", b"xab")]
    assert tops[:3] == [V, V, V] and tops[3] < V
    assert len(merges) == B.BOUNDARY_VOCAB - 256


@pytest.mark.parametrize("V", B.BOUNDARY_VS)
def test_boundary_to_exhaustion(V):
    counts = B.boundary(V, B.EXHAUST_WORDS)
    assert sum(counts.values()) == V and len(counts) == B.EXHAUST_WORDS
    assert list(counts) == list(B.boundary(V))[:B.EXHAUST_WORDS]
    assert {B.class_of(len(w)) for w in counts} == {0, 1, 2, 3, 4}
    vocab, merges, tops = B.tops(counts, B.EXHAUST_VOCAB)
    assert merges[:3] == [(b"x", b"a"), (b"xa", b"b"), (b" ", b"xab")]
    assert tops[:3] == [V, V, V] and tops[3] < V
    # no pair is left: every word is one token (the reference goes on to merge the pairs whose
    # count fell to zero, as its dict keeps them: more merges than the words have bytes)
    assert 300 < len(merges) < 3000
    assert all(w in vocab.values() for w in counts)


@pytest.mark.parametrize("V", B.BOUNDARY_VS)
def test_one_block(V):
    counts = B.one_block(V)
    assert counts[b" xab"] + counts[b" xabc"] == V
    assert (counts[b" xab"] & 0xFFFFFFFF) + (counts[b" xabc"] & 0xFFFFFFFF) >= (V & 0xFFFFFFFF)
    assert B.class_of(len(b" xab")) == B.class_of(len(b" xabc")) == 0
    assert sum(c for w, c in counts.items() if not w.startswith(b" xab")) < 1 << 20
    _vocab, merges, tops = B.tops(counts, B.BOUNDARY_VOCAB)
    assert merges[:3] == [(b"x", b"a"), (b"xa", b"b"), (b" ", b"xab")]
    assert tops[:3] == [V, V, V] and tops[3] < V
    assert len(merges) == B.BOUNDARY_VOCAB - 256


def test_near_limit():
    counts = B.near_limit()
    w = B.weight(counts)
    assert 1 << 61 <= w < 1 << 62
    assert w + B.weight(B.base_counts()) > B.WEIGHT_LIMIT - 1   # the largest factor
    assert B.train_counts(counts, B.VOCAB) == _oracle("synth")


def test_mixed_magnitudes():
    counts = B.mixed_magnitudes()
    base = B.base_counts()
    assert {counts[w] // c for w, c in base.items()} == set(B.MAGNITUDES)
    assert B.weight(counts) < B.WEIGHT_LIMIT
    seen = []
    _vocab, merges = B.train_counts(counts, B.VOCAB, (), lambda pairs, best: seen.append((best, pairs[best])))
    assert merges != _oracle("synth")[1]     # not a uniform scaling: only train_counts applies
    (a, b), top = seen[0]
    assert top >= 1 << 32
    small = [c * w.count(a + b) for w, c in counts.items() if c < 1 << 32 and a + b in w]   # (a != b)
    print(f"mixed_magnitudes: round 0 {(a, b)!r} count {top}, of which {sum(small)} in {len(small)} "
          f"words below 2^32; {sum(t >= 1 << 32 for _p, t in seen)} rounds at 2^32 or above")
    assert a != b and len(small) >= 100 and sum(small) >= 1 << 32
    assert sum(t >= 1 << 32 for _p, t in seen) >= 100
