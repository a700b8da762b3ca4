"""CPU: the deep-tie training inputs (tests/tie_cases.py).  The C oracle and the pure-Python
restatement of the reference trainer agree on them, and they still do what they are for: in
enough rounds the winner is told from the best tied runner-up only past the zero-padded 8-byte
prefix -- by a byte at index >= 8, or by the length ("\\x00" against "\\x00\\x00").  The counts
come from oracle/cpu_ref.py alone (its per-round callback), not from the code under test; over
seeds 0-3 they were 3-8 / 5-11 (prefix), 0 / 17-37 (nul) and 5-10 / 26-45 (nulstem) rounds
decided by byte / by length."""
import pytest

pytest.importorskip("regex")   # oracle/cpu_ref.py pre-tokenizes with it

import tie_cases  # noqa: E402
from oracle import cpu_ref  # noqa: E402
from oracle import oracle  # noqa: E402


@pytest.mark.parametrize("kind,seed", tie_cases.all_cases())
def test_oracle_matches_cpu_ref_on_deep_ties(kind, seed):
    text = tie_cases.case(seed, kind)
    vocab, merges, info = cpu_ref.train(text, tie_cases.VOCAB, [])
    assert info["complete"]
    o_vocab, o_merges = oracle.train_raw(text.encode("utf-8"), tie_cases.VOCAB, [])
    assert o_merges == merges
    assert o_vocab == vocab


@pytest.mark.parametrize("kind,seed", tie_cases.all_cases())
def test_cases_reach_the_deep_comparison(kind, seed):
    by_byte, by_len = tie_cases.deep_rounds(tie_cases.case(seed, kind), tie_cases.VOCAB)
    print(f"{kind} seed {seed}: {by_byte} rounds decided by a byte at index >= 8, {by_len} by length")
    if kind in ("prefix", "nulstem"):
        assert by_byte >= 3
    if kind in ("nul", "nulstem"):
        assert by_len >= 10


@pytest.mark.parametrize("kind", tie_cases.KINDS)
def test_scaled_cases_reach_the_deep_comparison(kind):
    text = tie_cases.case(0, kind, tie_cases.SCALED_WORDS)
    by_byte, by_len = tie_cases.deep_rounds(text, tie_cases.SCALED_VOCAB)
    print(f"{kind} scaled: {by_byte} rounds decided by a byte at index >= 8, {by_len} by length")
    if kind in ("prefix", "nulstem"):
        assert by_byte >= 3
    if kind in ("nul", "nulstem"):
        assert by_len >= 10
