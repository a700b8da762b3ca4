"""Encode with offsets on the GPU (bpe_tok_encode_spans*, Tokenizer.encode_with_offsets and the
batch forms): ids and spans, in bytes and in characters, compared exactly with the plain-Python
restatement tests/span_cases.py::spans_ref -- on the fixture texts, on every path of the emit, at
the character edges of the 64-byte blocks and 16 KiB chunks, around specials, over batches, through
offset device pointers and under the encoder's run-time paths."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

import emit_cases as ec
import span_cases as sc

pytestmark = pytest.mark.gpu

bpe_amd = pytest.importorskip("bpe_amd")
from bpe_amd import _lib  # noqa: E402

UNITS = ("byte", "char")


@functools.lru_cache(maxsize=None)
def _pair(which, specials=()):
    """(Tokenizer, SpanRef) of a named tokenizer"""
    if which == "gpt2":
        vocab, merges = sc.gpt2(tuple(specials))
    elif which == "small":
        vocab, merges = sc.small()
    else:
        vocab, merges = ec.vocab(), ec.merges()
    return (bpe_amd.Tokenizer(dict(vocab), list(merges), list(specials)),
            sc.SpanRef(dict(vocab), list(merges), list(specials)))


def _check_docs(tok, ref, docs, units=UNITS):
    docs = list(docs)
    for unit in units:
        ids, off, spans = tok.encode_batch_offsets_np(docs, unit)
        assert ids.dtype == np.uint32 and off.dtype == np.int64 and spans.dtype == np.int64
        assert off.shape == (len(docs) + 1,) and spans.shape == (ids.shape[0], 2)
        want_ids, want_spans, want_off = [], [], [0]
        for d in docs:
            i, s = ref.spans(d, unit)
            want_ids += i
            want_spans += s
            want_off.append(len(want_ids))
        assert off.tolist() == want_off
        assert ids.tolist() == want_ids
        got = [tuple(x) for x in spans.tolist()]
        if got != want_spans:
            k = next(j for j, (a, b) in enumerate(zip(got, want_spans)) if a != b)
            raise AssertionError(f"unit {unit}: span {k} is {got[k]}, want {want_spans[k]} (id {want_ids[k]})")


# ---------------------------------------------------------------------- fixture texts
def _fixture_docs():
    corpus = sc.fixture_text("corpus.en")
    return [sc.fixture_text("address.txt"), sc.fixture_text("german.txt"), corpus[:40000], corpus[50000:70000],
            sc.fixture_text("tinystories_sample.txt")[:60000]]


@pytest.mark.parametrize("which", ["gpt2", "small"])
@pytest.mark.parametrize("specials", [(), (sc.EOT,), tuple(sc.OVERLAPPING)], ids=["none", "eot", "overlapping"])
def test_fixture_texts(which, specials):
    tok, ref = _pair(which, specials)
    docs = _fixture_docs()
    if specials:
        docs = [d[:1000] + specials[-1] + d[1000:3000] + sc.EOT + sc.EOT + d[3000:] + sc.EOT for d in docs]
    _check_docs(tok, ref, docs)
    ids, spans = tok.encode_with_offsets(docs[1])
    assert (ids, spans) == ref.spans(docs[1], "char")
    assert ids == tok.encode(docs[1])


# ---------------------------------------------------------------------- the emit's paths
@pytest.mark.parametrize("case", sorted(ec.CASES))
def test_emit_paths(case):
    tok, ref = _pair("emit", tuple(ec.SPECIALS))
    _check_docs(tok, ref, [ec.CASES[case]()])


def test_word_load_tails():
    tok, ref = _pair("emit", tuple(ec.SPECIALS))
    _check_docs(tok, ref, list(ec.word_load_tails()))


def test_words_by_id_count():
    tok, ref = _pair("emit", tuple(ec.SPECIALS))
    text = sc.id_count_words()
    ids, spans = ref.spans(text, "byte")
    per_word = {}
    for (s, e) in spans:
        w = text.rfind(" ", 0, s + 1)
        per_word[w] = per_word.get(w, 0) + 1
    assert {1, 2, 3, 4, 5} <= set(per_word.values()) and max(per_word.values()) > 5
    _check_docs(tok, ref, [text])


# ---------------------------------------------------------------------- character edges
@pytest.mark.parametrize("boundary", [sc.K_BLOCK, 2 * sc.K_BLOCK, sc.K_CHUNK, 2 * sc.K_CHUNK])
def test_character_edges(boundary):
    tok, ref = _pair("small")
    _check_docs(tok, ref, [t for _, t in sc.char_edge_texts(boundary)])   # (later documents: other phases)
    for _, docs in sc.char_edge_batches(boundary):
        _check_docs(tok, ref, docs)
    for _, text in sc.char_edge_texts(boundary)[::4]:   # each text alone: its edge at that offset of the text
        _check_docs(tok, ref, [text])
    gtok, gref = _pair("gpt2")
    for _, text in sc.char_edge_texts(boundary)[::3]:
        _check_docs(gtok, gref, [text])


# ---------------------------------------------------------------------- specials
@pytest.mark.parametrize("case", sc.special_texts(), ids=[c[0] for c in sc.special_texts()])
@pytest.mark.parametrize("which", ["gpt2", "small"])
def test_specials(which, case):
    _, specials, text = case
    tok, ref = _pair(which, tuple(specials))
    _check_docs(tok, ref, [text])
    _check_docs(tok, ref, [text, "", text + " x", text])


# ---------------------------------------------------------------------- batches
@pytest.mark.parametrize("case", sc.seam_batches(), ids=[c[0] for c in sc.seam_batches()])
def test_batches(case):
    tok, ref = _pair("small", (sc.EOT,))
    _check_docs(tok, ref, case[1])


def test_many_documents():
    tok, ref = _pair("small", (sc.EOT,))
    docs = sc.sliced_batch()
    docs[17] = "naïve café " + sc.EOT + " 😀😀"
    _check_docs(tok, ref, docs)
    got = tok.encode_batch_offsets(docs[:50])
    assert got == [ref.spans(d, "char") for d in docs[:50]]


@pytest.mark.parametrize("text", sc.SHORT_TEXTS, ids=[str(len(t.encode())) for t in sc.SHORT_TEXTS])
def test_short_texts(text):
    tok, ref = _pair("small")
    assert len(text.encode()) in (0, 1, 2, 17)
    for unit in UNITS:
        assert tok.encode_with_offsets(text, unit) == ref.spans(text, unit)
    _check_docs(tok, ref, [text])


# ---------------------------------------------------------------------- device pointers, run-time paths
GUARD = 64


def _device_spans(tok, docs, unit, shift):
    """bpe_tok_encode_spans_device with the text at a pointer offset by `shift` bytes and guard
    elements around d_ids and d_spans; -> (ids, id offsets, spans)"""
    import torch
    data, starts = tok._join(docs)
    n, nd = len(data), len(docs)
    dev = torch.device("cuda", torch.cuda.current_device())
    buf = torch.zeros(n + shift + 64, dtype=torch.uint8, device=dev)
    buf[shift:shift + n] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    d_ids = torch.full((n + 2 * GUARD,), -7, dtype=torch.int32, device=dev)
    d_spans = torch.full((n + 2 * GUARD, 2), -9, dtype=torch.int32, device=dev)
    d_off = torch.zeros(nd + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    n_out = ctypes.c_size_t(0)
    rc = _lib.lib().bpe_tok_encode_spans_device(
        tok._device(), ctypes.c_void_p(buf.data_ptr() + shift), n, starts.ctypes.data, nd, sc_unit(unit),
        ctypes.c_void_p(d_ids.data_ptr() + 4 * GUARD), ctypes.byref(n_out), ctypes.c_void_p(d_off.data_ptr()),
        ctypes.c_void_p(d_spans.data_ptr() + 8 * GUARD), None)
    _lib.check(rc, "encode_spans_device")
    m = n_out.value
    ids, spans = d_ids.cpu().numpy(), d_spans.cpu().numpy()
    assert (ids[:GUARD] == -7).all() and (ids[GUARD + m:] == -7).all(), "d_ids written outside its ids"
    assert (spans[:GUARD] == -9).all() and (spans[GUARD + m:] == -9).all(), "d_spans written outside its spans"
    return (ids[GUARD:GUARD + m].astype(np.uint32).tolist(), d_off.cpu().tolist(),
            [tuple(x) for x in spans[GUARD:GUARD + m].astype(np.uint32).tolist()])


def sc_unit(unit):
    return {"byte": 0, "char": 1}[unit]


def _pointer_docs():
    corpus = sc.fixture_text("corpus.en")
    german = sc.fixture_text("german.txt")
    return [german[:3000], "", corpus[:sc.K_CHUNK + 3], "é" + corpus[20000:52000] + "€", sc.EOT + german[3000:9000], "😀"]


def _want(ref, docs, unit):
    ids, spans, off = [], [], [0]
    for d in docs:
        i, s = ref.spans(d, unit)
        ids += i
        spans += s
        off.append(len(ids))
    return ids, off, spans


@pytest.mark.parametrize("shift", [0, 1, 5, 15])
def test_device_pointers(shift):
    tok, ref = _pair("small", (sc.EOT,))
    docs = _pointer_docs()
    for unit in UNITS:
        assert _device_spans(tok, docs, unit, shift) == _want(ref, docs, unit)


RUNTIME_PATHS = [
    {"BPE355_ENC_PEND_CAP": "0"},                                # no pending pool: the scan resolves words
    {"BPE355_ENC_PEND_CAP": "40000", "BPE355_STREAM_WG": "2"},   # the pool runs out part way
    {"BPE355_ENC_FINALIZE": "0"},                                # the emit reads resolved records
    {"BPE355_ENC_TABLE_SLOTS": "65536"},                         # 40 000 distinct words: the table retry
    {"BPE355_ENC_REC_CAP": "1000"},                              # too few records: the record retry
]


@pytest.mark.parametrize("knobs", RUNTIME_PATHS, ids=["-".join(k) for k in RUNTIME_PATHS])
def test_runtime_paths(monkeypatch, knobs):
    import synth_text
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    tok, ref = _pair("small", (sc.EOT,))
    docs = [synth_text.generate(31, 200_000, "mixed"), sc.EOT, synth_text.generate(32, 120_000, "space") + sc.EOT,
            "", synth_text.generate(33, 150_000, "mixed"),
            " ".join(f"w{i:x}k{(i * 2654435761) % 997:x}" for i in range(40_000))]
    for unit in UNITS:
        assert _device_spans(tok, docs, unit, 5) == _want(ref, docs, unit)


# ---------------------------------------------------------------------- padded form
@pytest.mark.parametrize("truncation", ["right", "left"])
@pytest.mark.parametrize("padding_side", ["right", "left"])
def test_padded(truncation, padding_side):
    import torch
    tok, ref = _pair("small", (sc.EOT,))
    docs = ["", "a", "naïve café 😀 and more words here", sc.EOT, sc.fixture_text("german.txt")[:400], "x" * 3, ""]
    for T in (None, 8):
        for unit in UNITS:
            ids, lengths, spans = tok.encode_batch_padded_offsets(docs, T, pad_id=-3, truncation=truncation,
                                                                  padding_side=padding_side, unit=unit)
            pids, plen = tok.encode_batch_padded(docs, T, pad_id=-3, truncation=truncation, padding_side=padding_side)
            assert torch.equal(ids, pids) and torch.equal(lengths, plen)
            assert spans.dtype == torch.int64 and tuple(spans.shape) == tuple(ids.shape) + (2,)
            cids, off, cspans = tok.encode_batch_offsets_np(docs, unit)
            Tn = ids.shape[1]
            want = np.zeros((len(docs), Tn, 2), dtype=np.int64)
            for i in range(len(docs)):
                row = cspans[off[i]:off[i + 1]]
                kept = row[len(row) - min(len(row), Tn):] if truncation == "left" else row[:Tn]
                c0 = Tn - len(kept) if padding_side == "left" else 0
                want[i, c0:c0 + len(kept)] = kept
            assert np.array_equal(spans.cpu().numpy(), want)


# ---------------------------------------------------------------------- the other calls, shared ids, arguments
def test_other_calls_unchanged():
    import torch
    tok, _ = _pair("small", (sc.EOT,))
    docs = _pointer_docs()
    text = docs[3]
    before = (tok.encode(text), [a.tolist() for a in tok.encode_batch_np(docs)],
              [t.cpu().tolist() for t in tok.encode_batch_padded(docs, 16, pad_id=0)])
    tok.encode_batch_offsets_np(docs, "char")
    tok.encode_batch_padded_offsets(docs, 16, pad_id=0)
    after = (tok.encode(text), [a.tolist() for a in tok.encode_batch_np(docs)],
             [t.cpu().tolist() for t in tok.encode_batch_padded(docs, 16, pad_id=0)])
    assert before == after
    tok.release_device_buffers()
    assert tok.encode_with_offsets(text, "byte") == _pair("small", (sc.EOT,))[1].spans(text, "byte")
    torch.cuda.synchronize()


def test_shared_id_of_different_lengths_is_refused():
    vocab, merges, specials = sc.shared_len_vocab()
    tok = bpe_amd.Tokenizer(dict(vocab), list(merges), list(specials))
    text = "ab" + sc.EOT + "c"
    assert tok.encode(text) == [97, 98, 256, 99]   # plain encode is untouched
    for call in (lambda: tok.encode_with_offsets(text), lambda: tok.encode_batch_offsets_np([text], "byte"),
                 lambda: tok.encode_batch_padded_offsets([text], 4, pad_id=0)):
        with pytest.raises(ValueError, match="different lengths"):
            call()
    assert tok.encode(text) == [97, 98, 256, 99]


def test_shared_id_of_one_length_is_exact():
    vocab, merges, specials = sc.shared_same_len_vocab()
    tok = bpe_amd.Tokenizer(dict(vocab), list(merges), list(specials))
    text = "aZ bZ"
    ids, spans = tok.encode_with_offsets(text, "byte")
    assert ids == [97, 255, 32, 98, 255] and spans == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]
    assert (ids, spans) == sc.spans_ref(vocab, merges, specials, text, "byte")


def test_unknown_unit():
    tok, _ = _pair("small")
    for call in (lambda: tok.encode_with_offsets("abc", "bogus"), lambda: tok.encode_batch_offsets_np(["abc"], "bogus"),
                 lambda: tok.encode_batch_offsets(["abc"], None),
                 lambda: tok.encode_batch_padded_offsets(["abc"], 4, pad_id=0, unit="bytes")):
        with pytest.raises(ValueError):
            call()
    import torch
    d = torch.zeros(64, dtype=torch.int32, device="cuda")
    starts = np.zeros(1, dtype=np.uint64)
    n_out = ctypes.c_size_t(0)
    rc = _lib.lib().bpe_tok_encode_spans_device(tok._device(), ctypes.c_void_p(d.data_ptr()), 3, starts.ctypes.data, 1, 2,
                                                ctypes.c_void_p(d.data_ptr()), ctypes.byref(n_out),
                                                ctypes.c_void_p(d.data_ptr()), ctypes.c_void_p(d.data_ptr()), None)
    assert rc == _lib.BPE_E_ARG


def test_empty_batch():
    tok, _ = _pair("small")
    ids, off, spans = tok.encode_batch_offsets_np([])
    assert ids.shape == (0,) and off.tolist() == [0] and spans.shape == (0, 2)
    ids, off, spans = tok.encode_batch_offsets_np(["", ""])
    assert ids.shape == (0,) and off.tolist() == [0, 0, 0] and spans.shape == (0, 2)
    assert tok.encode_batch_offsets([]) == []
