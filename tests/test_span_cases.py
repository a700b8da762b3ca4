"""CPU-side checks of tests/span_cases.py: the restatement's ids are the oracle's and cpu_ref's, its
byte spans are the ids' vocab entries, its character spans contain them, and each input reaches
what it is built for (the emit's paths through tests/emit_cases.py's plan())."""
from __future__ import annotations

import pytest

import emit_cases as ec
import span_cases as sc
from oracle import oracle
from oracle.cpu_ref import Encoder


def _all_cases():
    """(name, which tokenizer, specials, text)"""
    out = []
    corpus = sc.fixture_text("corpus.en")
    for name in ("address.txt", "german.txt", "tinystories_sample.txt"):
        out.append((name, "small", [sc.EOT], sc.fixture_text(name)))
        out.append((name, "gpt2", [sc.EOT], sc.fixture_text(name)))
    out.append(("corpus-head", "small", [], corpus[:6000]))
    out.append(("corpus-head", "gpt2", [], corpus[:1500]))
    out += [(n, "small", [], t) for n, t in sc.char_edge_texts(sc.K_BLOCK)]
    out += [(n, "small", [], t) for n, t in sc.char_edge_texts(sc.K_CHUNK)[21:22]]   # a 4-byte straddler
    out += [(n, "small", sp, t) for n, sp, t in sc.special_texts()]
    out += [(n, "gpt2", sp, t) for n, sp, t in sc.special_texts()]
    out.append(("id-counts", "emit", ec.SPECIALS, sc.id_count_words()[:6000]))
    out += [(f"short{len(t.encode())}", "small", [], t) for t in sc.SHORT_TEXTS]
    return out


def _tokenizer(which, specials):
    if which == "gpt2":
        return sc.gpt2(tuple(specials))
    if which == "small":
        return sc.small()
    return ec.vocab(), ec.merges()


@pytest.mark.parametrize("case", _all_cases(), ids=lambda c: f"{c[1]}-{c[0]}")
def test_restatement(case):
    _, which, specials, text = case
    vocab, merges = _tokenizer(which, specials)
    data = text.encode("utf-8")
    ids, spans = sc.spans_ref(vocab, merges, specials, text, "byte")
    assert ids == Encoder(vocab, merges, specials).encode(text)
    assert ids == oracle.encode(vocab, merges, specials, text)
    ids_c, chars = sc.spans_ref(vocab, merges, specials, text, "char")
    assert ids_c == ids and len(spans) == len(ids) == len(chars)
    full = Encoder(vocab, merges, specials).vocab   # with the missing specials' bytes -> id entries
    special_bytes = {s.encode() for s in specials}
    prev = 0
    for i, (s, e), (a, b) in zip(ids, spans, chars):
        assert prev <= s < e <= len(data)
        prev = e
        piece = data[s:e]
        assert piece in special_bytes and full.get(piece, i) == i or vocab[i] == piece   # one-to-one vocabs
        assert piece in text[a:b].encode("utf-8")
        assert a == sc.char_index(data, s) - ((data[s] & 0xC0) == 0x80) and b == sc.char_index(data, e)
    if not specials:   # no dropped pre-token, no gap: the spans tile the text
        assert [s for s, _ in spans] == [0] + [e for _, e in spans][:-1] or not spans
        assert not spans or spans[-1][1] == len(data)


def test_split_characters_are_covered_by_both_tokens():
    vocab, merges = sc.small()
    text = "a€b"
    ids, spans = sc.spans_ref(vocab, merges, [], text, "byte")
    assert spans == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]          # the euro sign's bytes are three ids
    _, chars = sc.spans_ref(vocab, merges, [], text, "char")
    assert chars == [(0, 1), (1, 2), (1, 2), (1, 2), (2, 3)]


def test_unknown_unit():
    with pytest.raises(ValueError):
        sc.spans_ref(*sc.small(), [], "abc", "bogus")


def test_emit_cases_reach_their_paths():
    """the emit inputs the span kernel is run on hold the three write paths (plan() restates the
    split; tests/test_emit_cases.py checks each case in detail)"""
    seen, odd_first = set(), set()
    for name in ("path_b", "records_edge", "empty_chunks"):
        P = 0
        for _mc, parts in ec.plan(ec.CASES[name]()):
            for m, T in parts:
                path = "c" if m > ec.PART_RECORDS else "b" if T > ec.K_EMIT_IDS else "a"
                seen.add(path)
                if path == "a" and T:
                    odd_first.add(P % 2)   # an odd first id: the span store's one-span head
                P += T
    assert seen == {"a", "b", "c"} and odd_first == {0, 1}


def test_character_edges_reach_the_boundaries():
    for boundary in (sc.K_BLOCK, sc.K_CHUNK):
        starts = set()
        for name, text in sc.char_edge_texts(boundary):
            data = text.encode()
            at = next(i for i, b in enumerate(data) if b >= 0x80)
            starts.add((len(sc.CHARS[int(name[0])].encode()), at - boundary))
        assert starts == {(nb, d) for nb in (2, 3, 4) for d in range(-4, 5)}
        straddle = [(nb, d) for nb, d in starts if d < 0 < d + nb]
        assert len(straddle) == 1 + 2 + 3
        for _, docs in sc.char_edge_batches(boundary):
            assert len(docs[0].encode()) - boundary in (-1, 0, 1) and docs[0].encode()[-1] >= 0x80
    vocab, merges = sc.small()
    ids, spans = sc.spans_ref(vocab, merges, [], sc.char_edge_texts(64)[0][1], "char")
    assert len(set(spans)) < len(spans)   # some character is shared by several tokens


def test_batches_reach_the_seams():
    for name, docs in sc.seam_batches():
        if name.startswith("seam"):
            d = int(name[4:])
            lens = [len(x.encode()) for x in docs]
            assert lens[1] == sc.K_CHUNK + d and lens[1] + lens[2] == 2 * sc.K_CHUNK - d
            assert docs[0] == docs[3] == docs[5] == ""
    docs = sc.sliced_batch()
    assert len(docs) == 3000 and "" in docs


def test_words_by_id_count():
    words = {w for w in sc.id_count_words().split(" ") if w}
    counts = {ec.word_ids((" " + w).encode()) for w in words}
    assert {1, 2, 3, 4, 5} <= counts and max(counts) > 5
    # a vocab entry of several ids: the encoder's dictionary holds it with its ids in the dictionary's pool
    assert ec.word_ids((" " + ec.JK15).encode()) == 2 and len(" " + ec.JK15) == 16


def test_no_pretoken_equals_a_special():
    """encode() never meets a pre-token equal to a special (see span_cases.find_drop): the search
    finds none.  Handed one -- the special list swapped in behind the split's back -- the
    restatement drops it, and the next span starts past it."""
    assert sc.find_drop(4) is None
    vocab, merges = sc.small()
    ref = sc.SpanRef(vocab, merges, [])
    want_ids = ref.byte_spans("1")[0] + ref.byte_spans(" d")[0]
    ref.enc.special_tokens = ["bc"]
    ids, spans = ref.byte_spans("1bc d")
    assert ids == want_ids
    assert spans[0] == (0, 1) and spans[1][0] == 3 and spans[-1][1] == 5


def test_shared_id_vocabs():
    v, m, sp = sc.shared_len_vocab()
    inv = Encoder(v, m, sp).vocab_inv
    assert inv[sc.EOT.encode()] == inv[b"\xff"] == 256
    v, m, sp = sc.shared_same_len_vocab()
    inv = Encoder(v, m, sp).vocab_inv
    assert inv[b"Z"] == inv[b"\xff"] == 255
