"""CPU: the word-length training inputs (tests/word_length_cases.py).  The C oracle and the
pure-Python restatement of the reference trainer agree on them, and they still do what they are
for: words on both sides of every slot-class boundary and far past the last one, rewrites in
every class (several occurrences in one word among them), words that move down through every
class and end as one token, more token bytes than the device's first token pool holds, and, for
"runs" and "periodic", pairs that run out before the vocabulary is full.  Everything here comes
from the oracle, oracle/cpu_ref.py and plain Python, nothing from the code under test.

At vocab 1500, seed 0, the replay counted these rewrites in classes 0, 1, 2, 3 and the long table
(of which with more than one occurrence):
  random      56 (1),   124 (9),   263 (37),  349 (117), 2727 (958)
  runs       336 (8),   242 (52),  180 (85),   86 (67),   104 (95)
  periodic   309 (17),  106 (76),   53 (53),   43 (42),    80 (78)
and 15 to 54 moves for each of long table -> class 3 -> 2 -> 1 -> 0.  "runs" stops after 857 merges
and "periodic" after 437; "random" makes 946 617 bytes of tokens against a first pool of
64 * 4097 = 262 208.  The floor of 20 rewrites per class was set before these were counted: more
than the three words of one length could give by passing through a class once each.
"""
import functools
import time

import pytest

pytest.importorskip("regex")   # oracle/cpu_ref.py pre-tokenizes with it

import word_length_cases as W  # noqa: E402
from oracle import cpu_ref  # noqa: E402
from oracle import oracle  # noqa: E402


@functools.lru_cache(maxsize=None)
def _oracle(kind, seed, vocab):
    return oracle.train_raw(W.case(kind, seed).encode("utf-8"), vocab, [])


@functools.lru_cache(maxsize=None)
def _replay(kind):
    words = list(oracle.word_counts(W.case(kind, 0).encode("utf-8"), []))
    return W.replay_classes(words, _oracle(kind, 0, 1500)[1])


@pytest.mark.parametrize("vocab", [300, 1500])
@pytest.mark.parametrize("kind,seed", W.all_cases())
def test_oracle_matches_cpu_ref(kind, seed, vocab):
    text = W.case(kind, seed)
    assert len(text) <= 48 * sum(W.LENGTHS)
    vocab_py, merges_py, info = cpu_ref.train(text, vocab, [])
    assert info["complete"]
    o_vocab, o_merges = _oracle(kind, seed, vocab)
    assert o_merges == merges_py
    assert o_vocab == vocab_py


@pytest.mark.parametrize("seed", W.SEEDS)
def test_oracle_matches_cpu_ref_exhaustion_text(seed):
    """The text of the runs to exhaustion (one random word at each length from 1000 on)."""
    text = W.to_exhaustion("random", seed)
    vocab_py, merges_py, info = cpu_ref.train(text, 1500, [])
    assert info["complete"]
    assert oracle.train_raw(text.encode("utf-8"), 1500, []) == (vocab_py, merges_py)
    assert W.to_exhaustion("runs", seed) == W.case("runs", seed)
    assert W.to_exhaustion("periodic", seed) == W.case("periodic", seed)


@pytest.mark.parametrize("text_of", [W.case, W.to_exhaustion])
@pytest.mark.parametrize("kind,seed", W.all_cases())
def test_lengths_present(kind, seed, text_of):
    counts = oracle.word_counts(text_of(kind, seed).encode("utf-8"), [])
    lens = {len(w) for w in counts}
    if text_of is W.case:
        short = 1 if kind == "runs" else 0    # "runs" has two one-letter words
        assert len(counts) == 3 * len(W.LENGTHS) - short
    assert lens == set(W.LENGTHS)            # every pre-token is " " + word
    for B in (7, 15, 31, 63):
        assert B in lens and B + 1 in lens
    assert max(lens) >= 4097


@pytest.mark.parametrize("L", W.LENGTHS)
def test_single_length_case(L):
    counts = oracle.word_counts(W.single_length_case(L).encode("utf-8"), [])
    assert len(counts) == 3 and {len(w) for w in counts} == {L}
    assert sorted(counts.values()) == [1, 1, 3]


def test_many_long_case():
    text = W.many_long_case()
    counts = oracle.word_counts(text.encode("utf-8"), [])
    assert len(counts) == W.MANY_LONG_WORDS > 64 * 256
    assert min(map(len, counts)) >= 65 and max(map(len, counts)) <= 73
    assert 1_100_000 <= len(text) <= 1_300_000
    t0 = time.perf_counter()
    _vocab, merges = oracle.train_raw(text.encode("utf-8"), W.MANY_LONG_VOCAB, [])
    print(f"many_long_case: {len(text)} bytes, oracle {time.perf_counter() - t0:.2f} s")
    assert len(merges) == W.MANY_LONG_VOCAB - 256
    r = W.replay_classes(list(counts)[:200], merges)   # (a sample: the replay is slow)
    print(f"many_long_case, 200 words: rewrites per class {r['rewrites']}, transitions {r['transitions']}")
    assert r["rewrites"][4] and r["rewrites"][3] and r["transitions"].get((4, 3))


@pytest.mark.parametrize("kind", W.KINDS)
def test_every_class_is_rewritten(kind):
    r = _replay(kind)
    print(f"{kind}: rewrites per class {r['rewrites']}, with several occurrences {r['multi']}, "
          f"transitions {sorted(r['transitions'].items())}, long words that shrank to exactly 63 ids "
          f"{r['to_63']}, words ending as one token {r['single']}")
    for c in range(5):
        assert r["rewrites"][c] >= 20
        assert r["multi"][c] >= 1
    for t in [(4, 3), (3, 2), (2, 1), (1, 0)]:
        assert r["transitions"].get(t, 0) >= 1
    assert r["single"] >= 1


def test_token_pool_must_grow():
    vocab, _merges = _oracle("random", 0, 1500)
    longest = max(len(w) for w in oracle.word_counts(W.case("random", 0).encode("utf-8"), []))
    total = sum(len(t) for t in vocab.values())
    print(f"random: {total} token bytes, first pool {64 * longest}")
    assert total > 64 * longest >= 65536


@pytest.mark.parametrize("kind", ["runs", "periodic"])
def test_pairs_run_out_early(kind):
    vocab, merges = _oracle(kind, 0, 1500)
    print(f"{kind}: {len(merges)} merges of {1500 - 256}, longest token {max(map(len, vocab.values()))} bytes")
    assert 100 < len(merges) < 1500 - 256
    assert max(map(len, vocab.values())) > 63    # long tokens are in play when the pairs run out
