"""Encode with BPE-dropout on the GPU (bpe_tok_encode_dropout*, Tokenizer.encode_dropout and the
batch and padded forms) against tests/dropout_cases.py's DropoutRef: exact ids and offsets on the
fixtures, at the word lengths where the device path changes, at block and chunk edges, in batches,
through offset device pointers and in padded rows."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

import dropout_cases as dc
import span_cases as sc

pytestmark = pytest.mark.gpu

bpe_amd = pytest.importorskip("bpe_amd")
from bpe_amd import _lib  # noqa: E402

PS = (0, 0.1, 0.5, 0.9, 1)
SEEDS = (7, 2 ** 63 + 11)


@functools.lru_cache(maxsize=None)
def _pair(which, specials=()):
    """(Tokenizer, DropoutRef) of a named tokenizer"""
    if which == "gpt2":
        vocab, merges = dc.gpt2(tuple(specials))
    elif which == "small":
        vocab, merges = dc.small()
    elif which == "doubling":
        vocab, merges = dc.doubling()
    else:
        vocab, merges = dc.ec.vocab(), dc.ec.merges()
    return (bpe_amd.Tokenizer(dict(vocab), list(merges), list(specials)),
            dc.DropoutRef(dict(vocab), list(merges), list(specials)))


def _check(tok, ref, docs, p, seed, base=0):
    docs = list(docs)
    ids, off = tok.encode_batch_dropout_np(docs, p, seed, base)
    assert ids.dtype == np.uint32 and off.dtype == np.int64 and off.shape == (len(docs) + 1,)
    want = ref.encode_batch_dropout(docs, p, seed, base)
    flat = [x for row in want for x in row]
    assert off.tolist() == list(np.cumsum([0] + [len(r) for r in want]))
    assert ids.tolist() == flat
    return ids, off


# ---------------------------------------------------------------------- fixtures
@pytest.mark.parametrize("kind", ["none", "eot", "overlap"])
@pytest.mark.parametrize("which", ["gpt2", "small"])
@pytest.mark.parametrize("name", list(dc.FIXTURE_TEXTS))
def test_fixture_texts(name, which, kind):
    specials, text = dc.with_specials(dc.FIXTURE_TEXTS[name](), kind)
    tok, ref = _pair(which, tuple(specials))
    for p in PS:
        for seed in SEEDS:
            _check(tok, ref, [text], p, seed, 3)


@pytest.mark.parametrize("which", ["gpt2", "small"])
def test_p0_is_the_deterministic_encode(which):
    tok, _ = _pair(which, (dc.EOT,))
    docs = [dc.with_specials(get(), "eot")[1] for get in dc.FIXTURE_TEXTS.values()] + ["", "a"]
    ids, off = tok.encode_batch_dropout_np(docs, 0, 5, 9)
    ids0, off0 = tok.encode_batch_np(docs)
    assert ids.tolist() == ids0.tolist() and off.tolist() == off0.tolist()
    for t in docs[:2]:
        assert tok.encode_dropout(t, 0, 123) == tok.encode(t)


# ---------------------------------------------------------------------- word lengths
@pytest.mark.parametrize("which", ["gpt2", "small"])
def test_word_lengths(which):
    tok, ref = _pair(which)
    docs = [w for _, w in dc.word_length_docs()]
    for p in PS:
        _check(tok, ref, docs, p, 7)
    _check(tok, ref, [" ".join(docs)], 0.5, 8)   # the same words as the pre-tokens of one document


@pytest.mark.parametrize("n", dc.LONG_AS)
def test_long_runs_of_one_letter(n):
    tok, ref = _pair("doubling")
    docs = ["a" * n, " é" + "a" * n + "é"]
    _check(tok, ref, docs, 0, 1)
    _check(tok, ref, docs, 0.5, 1)
    if n < 10000:
        _check(tok, ref, ["b" + "a" * n, "a" * n], 0.1, 2)


# ---------------------------------------------------------------------- block and chunk edges
@pytest.mark.parametrize("boundary", [dc.K_BLOCK, dc.K_CHUNK])
def test_words_at_edges(boundary):
    tok, ref = _pair("emit", (dc.EOT,))
    for _, text, _ in dc.edge_texts(boundary):
        for p in (0, 0.5, 0.9):
            _check(tok, ref, [text], p, 7)
    _check(tok, ref, [t for _, t, _ in dc.edge_texts(boundary)], 0.5, 9, 100)


# ---------------------------------------------------------------------- specials, repeated pairs
def test_special_texts():
    for _, specials, text in sc.special_texts():
        tok, ref = _pair("gpt2", tuple(specials))
        for p in (0, 0.5, 1):
            _check(tok, ref, [text, "", text + " tail"], p, 3)


def test_repeated_pair_keeps_its_last_index():
    vocab, merges, text, want = dc.repeated_pair()
    tok = bpe_amd.Tokenizer(vocab, merges, [])
    ref = dc.DropoutRef(vocab, merges, [])
    assert tok.encode_dropout(text, 0, 1) == want
    for seed in range(8):
        assert tok.encode_dropout(text * 20, 0.5, seed) == ref.encode_dropout(text * 20, 0.5, seed)


def test_known_answers():
    tok, _ = _pair("doubling")
    for (seed, key), want in dc.AAAA.items():
        assert tok.encode_dropout("aaaa aaaa", 0.5, seed, key) == want


# ---------------------------------------------------------------------- batches
def test_batches_and_document_keys():
    tok, ref = _pair("gpt2", (dc.EOT,))
    corpus = dc.fixture_text("corpus.en")
    for docs in ([corpus[:700]], ["", corpus[:700]], [corpus[:300], ""], ["", "", corpus[:200], "", "", corpus[200:900], ""],
                 ["", "", ""], []):
        _check(tok, ref, docs, 0.5, 7, 40)
    for _, docs in sc.seam_batches()[3:6]:
        _check(tok, ref, docs, 0.5, 7, 1)
    # row i of a batch is the document alone under its key
    docs = [corpus[:500], "", corpus[500:900], corpus[:500]]
    base = 1234
    rows = tok.encode_batch_dropout(docs, 0.5, 9, base)
    for i, t in enumerate(docs):
        assert rows[i] == tok.encode_dropout(t, 0.5, 9, doc_key=base + i)
    # the same document at two positions differs only through its key
    assert rows[0] != rows[3]
    assert rows[3] == tok.encode_batch_dropout([docs[3]], 0.5, 9, base + 3)[0]
    # keys near 2^64
    top = 2 ** 64 - 1 - len(docs)
    _check(tok, ref, docs, 0.5, 2 ** 64 - 1, top)


def test_3000_documents():
    tok, ref = _pair("gpt2", (dc.EOT,))
    docs = sc.sliced_batch(3000)
    docs[0] = docs[-1] = docs[1500] = docs[1501] = ""
    _check(tok, ref, docs, 0.3, 5, 10 ** 12)


# ---------------------------------------------------------------------- device pointers
GUARD = 64


def _device_dropout(tok, docs, p, seed, base, shift):
    """bpe_tok_encode_dropout_device with the text at a pointer offset by `shift` bytes and guard
    elements around the n entries of d_ids; -> (ids, id offsets)"""
    import torch
    data, starts = tok._join(docs)
    n, nd = len(data), len(docs)
    dev = torch.device("cuda", torch.cuda.current_device())
    buf = torch.zeros(n + shift + 64, dtype=torch.uint8, device=dev)
    buf[shift:shift + n] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    d_ids = torch.full((n + 2 * GUARD,), -7, dtype=torch.int32, device=dev)
    d_off = torch.zeros(nd + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    n_out = ctypes.c_size_t(0)
    rc = _lib.lib().bpe_tok_encode_dropout_device(
        tok._device(), ctypes.c_void_p(buf.data_ptr() + shift), n, starts.ctypes.data, nd, dc.thr_of(p), seed, base,
        ctypes.c_void_p(d_ids.data_ptr() + 4 * GUARD), ctypes.byref(n_out), ctypes.c_void_p(d_off.data_ptr()), None)
    _lib.check(rc, "encode_dropout_device")
    m = n_out.value
    ids = d_ids.cpu().numpy()
    assert (ids[:GUARD] == -7).all() and (ids[GUARD + n:] == -7).all(), "d_ids written outside its n entries"
    return ids[GUARD:GUARD + m].astype(np.uint32).tolist(), d_off.cpu().tolist()


@pytest.mark.parametrize("shift", [0, 1, 5, 15])
def test_offset_device_pointers(shift):
    tok, ref = _pair("gpt2", (dc.EOT,))
    corpus = dc.fixture_text("corpus.en")
    german = dc.fixture_text("german.txt")
    docs = [german[:3000], "", corpus[:dc.K_CHUNK + 3], "é" + corpus[20000:40000] + "€", dc.EOT + german[3000:6000],
            "😀", " " + "-" * 100]
    want = ref.encode_batch_dropout(docs, 0.5, 7, 2)
    ids, off = _device_dropout(tok, docs, 0.5, 7, 2, shift)
    assert ids == [x for r in want for x in r]
    assert off == list(np.cumsum([0] + [len(r) for r in want]))


def test_abi_argument_errors():
    import torch
    tok, _ = _pair("small")
    d = torch.zeros(64, dtype=torch.uint8, device="cuda")
    starts = np.zeros(1, dtype=np.uint64)
    n_out = ctypes.c_size_t(0)
    L = _lib.lib()

    def call(thr, base, nd=1):
        return L.bpe_tok_encode_dropout_device(tok._device(), ctypes.c_void_p(d.data_ptr()), 3, starts.ctypes.data, nd, thr,
                                               0, base, ctypes.c_void_p(d.data_ptr() + 16), ctypes.byref(n_out),
                                               ctypes.c_void_p(d.data_ptr() + 32), None)
    assert call(2 ** 24 + 1, 0) == _lib.BPE_E_ARG
    assert call(0, 2 ** 64 - 1) == _lib.BPE_E_ARG
    assert call(2 ** 24, 2 ** 64 - 2) == _lib.BPE_OK and n_out.value == 3


# ---------------------------------------------------------------------- padded rows
@pytest.mark.parametrize("truncation", ["right", "left"])
@pytest.mark.parametrize("padding_side", ["right", "left"])
def test_padded_rows_are_the_packed_csr(truncation, padding_side):
    import torch
    tok, _ = _pair("gpt2", (dc.EOT,))
    corpus = dc.fixture_text("corpus.en")
    docs = [corpus[:200], "", corpus[200:260], dc.EOT, corpus[300:1500]]
    ids, off = tok.encode_batch_dropout_np(docs, 0.5, 3, 50)
    rows = [ids[a:b].tolist() for a, b in zip(off, off[1:])]
    for dtype in (torch.int32, torch.int64):
        for T in (None, 16):
            out, lengths = tok.encode_batch_padded_dropout(docs, T, pad_id=-3, p=0.5, seed=3, doc_base=50,
                                                           truncation=truncation, padding_side=padding_side, dtype=dtype)
            width = max(map(len, rows)) if T is None else T
            assert out.dtype == dtype and out.is_cuda and tuple(out.shape) == (len(docs), width)
            assert lengths.tolist() == [min(len(r), width) for r in rows]
            for i, r in enumerate(rows):
                kept = r[:width] if truncation == "right" else r[len(r) - min(len(r), width):]
                pad = [-3] * (width - len(kept))
                assert out[i].tolist() == (kept + pad if padding_side == "right" else pad + kept)
    out, lengths = tok.encode_batch_padded_dropout([], 4, pad_id=0, p=0.5, seed=1)
    assert tuple(out.shape) == (0, 4) and lengths.numel() == 0


# ---------------------------------------------------------------------- KeyError, a large text
def test_missing_ids_raise_key_error():
    vocab, merges = dc.doubling()
    no_byte = {i: b for i, b in vocab.items() if b != b"q"}
    tok = bpe_amd.Tokenizer(no_byte, merges, [])
    with pytest.raises(KeyError):
        tok.encode("aq")
    with pytest.raises(KeyError):
        tok.encode_dropout("aaaa q", 0.5, 1)
    assert tok.encode_dropout("aaaa b", 0, 1) == [257, 32, 98]
    no_product = {i: b for i, b in vocab.items() if b != b"aa"}
    tok = bpe_amd.Tokenizer(no_product, merges, [])
    with pytest.raises(KeyError):
        tok.encode("aa")
    with pytest.raises(KeyError):
        tok.encode_dropout("aa " * 40, 0.5, 1)          # some occurrence keeps its merge
    assert tok.encode_dropout("aa aaaa", 1, 1) == [97, 97, 32, 97, 97, 97, 97]   # every byte: no product needed
    ref = dc.DropoutRef(no_product, merges, [])
    with pytest.raises(KeyError):
        ref.encode_dropout("a" * 100, 0.5, 1)
    with pytest.raises(KeyError):
        tok.encode_dropout("a" * 100, 0.5, 1)   # the long path


def test_one_megabyte_round_trips():
    tok, _ = _pair("gpt2", (dc.EOT,))
    base = dc.fixture_text("corpus.en")
    text = (base + dc.EOT) * (1_000_000 // (len(base) + len(dc.EOT)) + 1)
    text = text[:1_000_000]
    n0 = len(tok.encode(text))
    n_bytes = len(text.encode("utf-8"))
    for p in (0.1, 0.9):
        ids = tok.encode_dropout(text, p, 7)
        assert tok.decode(ids) == text
        assert n0 <= len(ids) <= n_bytes
