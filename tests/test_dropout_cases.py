"""CPU checks of the BPE-dropout restatement (tests/dropout_cases.py) and of the inputs built for
the device path: the known answers, p = 0 and p = 1, round trips, the dropped share of the draws,
and that every built case reaches the threshold it names."""
import math

import pytest

import dropout_cases as dc
from oracle.cpu_ref import Encoder


def test_known_draws():
    for args, want in dc.DRAWS:
        assert dc.draw_of(*args) == want, args


def test_known_thresholds():
    for p, want in dc.THRS.items():
        assert dc.thr_of(p) == want


def test_known_aaaa():
    vocab, merges = dc.doubling()
    assert len(merges) == 6 and vocab[256] == b"aa" and vocab[261] == b"a" * 64
    ref = dc.DropoutRef(vocab, merges, [])
    for (seed, key), want in dc.AAAA.items():
        assert ref.encode_dropout("aaaa aaaa", 0.5, seed, key) == want, (seed, key)


def test_repeated_pair_keeps_last_index():
    vocab, merges, text, want = dc.repeated_pair()
    assert dc.DropoutRef(vocab, merges, []).encode_dropout(text, 0, 5) == want
    assert Encoder(vocab, merges, []).encode(text) == want


@pytest.mark.parametrize("tok", ["gpt2", "small"])
@pytest.mark.parametrize("kind", ["none", "eot", "overlap"])
def test_p0_is_encode_and_p1_is_bytes(tok, kind):
    for name, get in dc.FIXTURE_TEXTS.items():
        specials, text = dc.with_specials(get()[:6000], kind)
        vocab, merges = dc.gpt2(tuple(specials)) if tok == "gpt2" else dc.small()
        ref = dc.DropoutRef(vocab, merges, specials)
        assert ref.encode_dropout(text, 0, 3, 9) == ref.encode(text), name
        ids = ref.encode_dropout(text, 1, 3, 9)
        n_sp = sum(1 for _, _, special in ref.pretokens_at(text) if special)
        sp_bytes = sum(len(s.encode()) for _, s, special in ref.pretokens_at(text) if special)
        assert len(ids) == len(text.encode()) - sp_bytes + n_sp, name
        assert ref.decode(ids) == text, name


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_round_trip(p):
    vocab, merges = dc.gpt2((dc.EOT,))
    ref = dc.DropoutRef(vocab, merges, [dc.EOT])
    for name, get in dc.FIXTURE_TEXTS.items():
        _, text = dc.with_specials(get()[:8000], "eot")
        assert ref.decode(ref.encode_dropout(text, p, 11, 2)) == text, name


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_dropped_share(p):
    """the draws are those of the ranked adjacent pairs, one per pair and round; their dropped
    share must lie within 4 sigma of p"""
    vocab, merges = dc.gpt2((dc.EOT,))
    ref = dc.DropoutRef(vocab, merges, [dc.EOT])
    ref.encode_dropout(dc.stats_text(), p, 7)
    n, k = ref.n_draws, ref.n_dropped
    z = (k - n * p) / math.sqrt(n * p * (1 - p))
    print(f"p={p}: {n} draws, {k} dropped, z = {z:+.2f}")
    assert n > 50_000 and abs(z) <= 4


def test_result_depends_on_seed_key_and_offset_only():
    vocab, merges = dc.gpt2(())
    ref = dc.DropoutRef(vocab, merges, [])
    text = dc.fixture_text("corpus.en")[:3000]
    a = ref.encode_dropout(text, 0.5, 1, 4)
    assert a == ref.encode_batch_dropout(["x", text], 0.5, 1, 3)[1]
    assert a != ref.encode_dropout(text, 0.5, 2, 4) and a != ref.encode_dropout(text, 0.5, 1, 5)


# ---------------------------------------------------------------------- the built cases
def test_word_length_docs_are_single_pretokens_of_their_length():
    k = dc.short_bound()
    assert k == 32
    vocab, merges = dc.gpt2(())
    enc = Encoder(vocab, merges, [])
    docs = dc.word_length_docs()
    seen = {n for n, _ in docs}
    assert seen == set(dc.word_lengths()) and {k - 1, k, k + 1} <= seen
    for n, w in docs:
        assert len(w.encode()) == n and enc.pretokenize(w) == [w], (n, w)
    for n in dc.word_lengths():
        if n >= 9:   # every form fits: leading space or not, each character at both ends
            forms = [w for m, w in docs if m == n]
            assert len(forms) == 8
            assert all(any(w.startswith(pre + ch) and w.endswith(ch) for w in forms)
                       for pre in ("", " ") for ch in dc.CHARS.values())


@pytest.mark.parametrize("boundary", [dc.K_BLOCK, dc.K_CHUNK])
def test_edge_texts_place_the_word(boundary):
    vocab, merges, specials = dc.emit_tokenizer()
    ref = dc.DropoutRef(vocab, merges, specials)
    names = set()
    for name, text, (start, end) in dc.edge_texts(boundary):
        at = {off: s for off, s, _ in ref.pretokens_at(text)}
        assert start in at and len(at[start].encode()) == end - start, name
        if "ends-at" in name:
            assert end == boundary
        elif "starts-at" in name:
            assert start == boundary
        else:
            assert start < boundary < end
        assert ("long" in name) == (end - start > dc.short_bound())
        names.add(name)
    assert len(names) == 6


def test_long_as_take_the_long_path_and_many_rounds():
    vocab, merges = dc.doubling()
    ref = dc.DropoutRef(vocab, merges, [])
    for n in dc.LONG_AS:
        assert n > dc.short_bound() and ref.pretokens_at("a" * n) == [(0, "a" * n, False)]
    ids = ref.encode_dropout("a" * 4097, 0, 1)
    assert ids == [261] * 64 + [97]
    ids = ref.encode_dropout("a" * 4097, 0.5, 1)
    assert ref.decode(ids) == "a" * 4097 and 65 < len(ids) < 4097


def test_special_texts_and_overlapping():
    for name, specials, text in dc.sc.special_texts():
        vocab, merges = dc.gpt2(tuple(specials))
        ref = dc.DropoutRef(vocab, merges, specials)
        assert ref.encode_dropout(text, 0, 1) == ref.encode(text), name
        assert ref.decode(ref.encode_dropout(text, 0.5, 1)) == text, name
