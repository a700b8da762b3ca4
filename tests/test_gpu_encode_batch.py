"""Tokenizer.encode_batch / encode_batch_np / encode_batch_padded (bpe_tok_encode_batch*,
bpe_ids_pack_rows_device): a list of documents encoded in one launch sequence, each document
exactly as a separate encode() -- checked per document against the oracle -- with the id offset of
every document start, and the ids packed into padded rows on the device.

The cases put document seams where joining the texts would change the ids (trailing whitespace,
contractions, a special token split by a seam), on and next to the encoder's 16 KiB chunk
boundaries, and into chunks with more records than one round of the offsets pass holds.
"""
from __future__ import annotations

import ctypes
import functools
import random

import numpy as np
import pytest

import golden_cases as G
import gpt2_files
from oracle import oracle

pytestmark = pytest.mark.gpu

bpe_amd = pytest.importorskip("bpe_amd")
from bpe_amd import _lib  # noqa: E402

EOT = ["<|endoftext|>"]
CH = 16384


@functools.lru_cache(maxsize=None)
def _inputs(which):
    if which == "t500":
        return gpt2_files.load_reference_train_golden()
    return gpt2_files.load_gpt2(EOT)


@functools.lru_cache(maxsize=None)
def _tok(which):
    vocab, merges = _inputs(which)
    return bpe_amd.Tokenizer(dict(vocab), list(merges), EOT)


def _ascii_corpus():
    text = (gpt2_files.FIXTURES / "corpus.en").read_text(encoding="utf-8")
    return "".join(c for c in text if ord(c) < 128)


@functools.lru_cache(maxsize=None)
def _seam_docs():
    fill = _ascii_corpus()
    docs = ["", "", "a", "", "", "a  ", "b", "don", "'t", "x<|endof", "text|>y", "<|endoftext|>", "",
            "café", "s", "世界", " <|endoftext|>", "<|endoftext|> z", "q"]
    at = [0]   # bytes so far / the filler consumed

    def size():
        return sum(len(d.encode("utf-8")) for d in docs)

    def fill_to(end):   # a filler document that ends exactly at byte `end` of the join
        k = end - size()
        assert k > 0
        docs.append(fill[at[0]:at[0] + k])
        at[0] += k

    for edge in (CH, 2 * CH):   # seams at edge - 1, edge, edge + 1
        fill_to(edge - 1)
        docs.append("x")
        docs.append(" ")
        assert size() == edge + 1
    fill_to(3 * CH)   # a document ending exactly on a chunk boundary, the next one starting there
    fill_to(3 * CH + 700)
    docs += ["", ""]
    ends = np.cumsum([len(d.encode("utf-8")) for d in docs]).tolist()
    for e in (CH - 1, CH, CH + 1, 2 * CH - 1, 2 * CH, 2 * CH + 1, 3 * CH):
        assert e in ends
    return tuple(docs)


@functools.lru_cache(maxsize=None)
def _many_docs():
    text = _ascii_corpus()
    text = (text * (400_000 // len(text) + 1))[:400_000]
    rng = random.Random(20240607)
    docs, p = [], 0
    while p < len(text):
        k = rng.choice((0, 1, 2, 5, 17, 40, 100, 300))
        docs.append(text[p:p + k])
        p += k
    return tuple(docs)


def _cut(text, n_cuts, seed):
    rng = random.Random(seed)
    cuts = sorted(rng.sample(range(1, len(text)), n_cuts))
    return tuple(text[a:b] for a, b in zip([0] + cuts, cuts + [len(text)]))


@functools.lru_cache(maxsize=None)
def _dense_docs():
    """32 KiB of single letters separated by spaces (8192 pre-tokens per 16 KiB chunk, 4096 records
    per chunk part), then 32 KiB of alternating letters and digits (a pre-token per byte, 8192 per
    part): parts of two and of four rounds of the offsets pass, past the emit's register path"""
    letters = "abcdefghijklmnopqrstuvwxyz"
    text = "".join(letters[(7 * i) % 26] + " " for i in range(16384))
    text += "".join(letters[(5 * i) % 26] + "0123456789"[(3 * i) % 10] for i in range(16384))
    return _cut(text, 50, 5)


@functools.lru_cache(maxsize=None)
def _distinct_docs():
    """40 000 distinct words, none in the 500-entry vocab's dictionary: more than half of a
    65536-slot word table, which the encoder then retries four times as large"""
    text = " ".join(f"w{i:x}k{(i * 2654435761) % 997:x}" for i in range(40_000))
    return _cut(text, 200, 6)


CASES = {
    "seams-t500": ("t500", _seam_docs),
    "seams-gpt2": ("gpt2", _seam_docs),
    "many": ("t500", _many_docs),
    "dense": ("t500", _dense_docs),
    "distinct": ("t500", _distinct_docs),
}


@functools.lru_cache(maxsize=None)
def _want(case):
    """the oracle's ids of every document, computed once per case and shared (read-only)"""
    which, docs = CASES[case]
    vocab, merges = _inputs(which)
    memo = {}
    rows = []
    for d in docs():
        if d not in memo:
            memo[d] = tuple(oracle.encode(vocab, merges, EOT, d))
        rows.append(memo[d])
    return tuple(rows)


def _chunks_ids(tok, docs):
    """bpe_tok_encode_chunks on the join with the documents' starts"""
    datas = [d.encode("utf-8") for d in docs]
    data = b"".join(datas)
    starts = np.cumsum([0] + [len(b) for b in datas[:-1]]).astype(np.uint64)
    out = (ctypes.c_uint32 * max(1, len(data)))()
    n_out = ctypes.c_size_t(0)
    _lib.check(_lib.lib().bpe_tok_encode_chunks(tok._device(), data, len(data), starts.ctypes.data, len(starts),
                                                out, len(data), ctypes.byref(n_out)))
    return list(out[:n_out.value])


def _check_case(case):
    which, docs = CASES[case]
    docs, want = docs(), _want(case)
    tok = _tok(which)
    ids, offsets = tok.encode_batch_np(list(docs))
    assert ids.dtype == np.uint32 and offsets.dtype == np.int64 and offsets.shape == (len(docs) + 1,)
    lens = [len(r) for r in want]
    assert offsets.tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist()
    flat = ids.tolist()
    assert len(flat) == sum(lens)
    off = offsets.tolist()
    for i, row in enumerate(want):
        assert tuple(flat[off[i]:off[i + 1]]) == row, (i, docs[i][:40])
    assert flat == _chunks_ids(tok, docs)


@pytest.mark.parametrize("case", ["seams-t500", "seams-gpt2"])
def test_seams(case):
    docs = _seam_docs()
    assert docs[0] == "" and docs[-1] == "" and docs[-2] == ""
    _check_case(case)
    which, _ = CASES[case]
    assert _tok(which).encode_batch(list(docs)) == [list(r) for r in _want(case)]


def test_many_documents():
    docs, want = _many_docs(), _want("many")
    assert 6000 < len(docs) < 9000
    vocab, merges = _inputs("t500")
    # encoding the join and splitting it afterwards cannot give these rows: the join's ids differ
    joined = oracle.encode(vocab, merges, EOT, "".join(docs))
    assert joined != [i for r in want for i in r]
    _check_case("many")


def test_dense_records():
    docs = _dense_docs()
    data = "".join(docs)
    assert len(data) == 65536 and len(docs) == 51
    assert len(data[:32768].split()) == 16384 and data[32768:].isalnum()
    _check_case("dense")


VARIANTS = [
    {"BPE355_ENC_FINALIZE": "0"},
    {"BPE355_ENC_FINALIZE": "2"},
    {"BPE355_ENC_PEND_CAP": "0"},
    {"BPE355_STREAM_WG": "1"},
    {"BPE355_ENC_REC_CAP": "1"},          # the record retry
    {"BPE355_ENC_TABLE_SLOTS": "65536"},  # with the distinct-words case: the table retry
]


@pytest.mark.parametrize("case", ["seams-t500", "seams-gpt2", "many", "dense", "distinct"])
@pytest.mark.parametrize("knobs", VARIANTS, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()))
def test_encoder_variants(monkeypatch, knobs, case):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    _check_case(case)


def test_distinct_words_default():
    assert len(set(" ".join(_distinct_docs()).split())) > 32768
    _check_case("distinct")


def _batch_rc(tok, data, starts):
    starts = np.asarray(starts, dtype=np.uint64)
    out = np.empty(max(1, len(data)), dtype=np.uint32)
    offs = np.empty(len(starts) + 1, dtype=np.uint64)
    n_out = ctypes.c_size_t(0)
    rc = _lib.lib().bpe_tok_encode_batch(tok._device(), data, len(data), starts.ctypes.data, len(starts),
                                         out.ctypes.data, out.size, ctypes.byref(n_out), offs.ctypes.data)
    return rc, out[:n_out.value].tolist(), offs.tolist()


@pytest.mark.parametrize("starts", [[1, 4], [0, 6, 3], [0, 4, 12]],
                         ids=["first-not-0", "decreasing", "past-the-end"])
def test_argument_errors(starts):
    tok = _tok("t500")
    data = b"hello world"
    rc, _, _ = _batch_rc(tok, data, starts)
    assert rc == _lib.BPE_E_ARG
    with pytest.raises(RuntimeError):
        _lib.check(rc, "encode_batch")
    # the tokenizer is still usable
    rc, ids, offs = _batch_rc(tok, data, [0, 5, 11])
    vocab, merges = _inputs("t500")
    a, b = oracle.encode(vocab, merges, EOT, "hello"), oracle.encode(vocab, merges, EOT, " world")
    assert rc == 0 and ids == a + b and offs == [0, len(a), len(a) + len(b), len(a) + len(b)]


def test_empty_inputs():
    tok = _tok("t500")
    ids, offsets = tok.encode_batch_np([])
    assert ids.shape == (0,) and offsets.tolist() == [0]
    assert tok.encode_batch([]) == []
    assert tok.encode_batch(["", "", ""]) == [[], [], []]   # no text at all: no launch
    ids, offsets = tok.encode_batch_np(["", ""])
    assert ids.shape == (0,) and offsets.tolist() == [0, 0, 0]


# ---------------------------------------------------------------------- padded rows
def _pad_want(ids, offsets, T, pad, truncation, padding_side, dtype):
    B = len(offsets) - 1
    out = np.full((B, T), pad, dtype=dtype)
    lengths = np.zeros(B, dtype=np.int32)
    for i in range(B):
        row = ids[offsets[i]:offsets[i + 1]]
        row = row[:T] if truncation == "right" else row[len(row) - min(len(row), T):]
        lengths[i] = len(row)
        if padding_side == "right":
            out[i, :len(row)] = row
        else:
            out[i, T - len(row):] = row
    return out, lengths


def _texts_with_lengths(tok, lengths):
    """texts whose id counts are exactly `lengths`: one-byte words of the byte vocab"""
    texts = ["".join("abcdefg"[(i + j) % 7] + " " for j in range(L // 2)) + ("z" if L % 2 else "")
             for i, L in enumerate(lengths)]
    return texts


@functools.lru_cache(maxsize=None)
def _byte_tok():
    return bpe_amd.Tokenizer({i: bytes([i]) for i in range(256)}, [], [])


@pytest.mark.parametrize("dtype", ["int32", "int64"])
@pytest.mark.parametrize("padding_side", ["right", "left"])
@pytest.mark.parametrize("truncation", ["right", "left"])
@pytest.mark.parametrize("T", [8, 7])   # 16-byte stores / element stores (a row is no multiple of 16 bytes)
def test_padded_rows(T, truncation, padding_side, dtype):
    import torch
    tok = _byte_tok()
    texts = _texts_with_lengths(tok, [0, 1, T - 1, T, T + 1, 3 * T, 2, 0])
    ids, offsets = tok.encode_batch_np(texts)
    assert np.diff(offsets).tolist() == [0, 1, T - 1, T, T + 1, 3 * T, 2, 0]
    tdt = getattr(torch, dtype)
    got, lengths = tok.encode_batch_padded(texts, T, pad_id=-7, truncation=truncation, padding_side=padding_side,
                                           dtype=tdt)
    assert got.dtype == tdt and got.shape == (len(texts), T) and got.is_cuda
    assert lengths.dtype == torch.int32 and lengths.is_cuda
    want, wlen = _pad_want(ids.astype(np.int64), offsets, T, -7, truncation, padding_side, np.dtype(dtype))
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(lengths.cpu().numpy(), wlen)


def test_padded_real_text_max_length_none():
    import torch
    tok = _tok("t500")
    texts = list(_many_docs()[:300])
    ids, offsets = tok.encode_batch_np(texts)
    T = int(np.diff(offsets).max())
    got, lengths = tok.encode_batch_padded(texts, pad_id=0)
    assert got.dtype == torch.int64 and got.shape == (300, T)
    want, wlen = _pad_want(ids.astype(np.int64), offsets, T, 0, "right", "right", np.int64)
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(lengths.cpu().numpy(), wlen)
    got, lengths = tok.encode_batch_padded([], 16, pad_id=0)
    assert got.shape == (0, 16) and lengths.shape == (0,)
    got, lengths = tok.encode_batch_padded(["", ""], pad_id=0)
    assert got.shape == (2, 0) and lengths.tolist() == [0, 0]
    with pytest.raises(ValueError):
        tok.encode_batch_padded(texts, 8, pad_id=0, truncation="middle")
    with pytest.raises(ValueError):
        tok.encode_batch_padded(texts, 8, pad_id=0, dtype=torch.float32)


@pytest.mark.parametrize("truncation,padding_side", [("right", "left"), ("left", "right")])
def test_padded_one_long_row(truncation, padding_side):
    import torch
    tok = _byte_tok()
    texts = _texts_with_lengths(tok, [5000])
    ids, offsets = tok.encode_batch_np(texts)
    assert offsets.tolist() == [0, 5000]
    for T in (4096, 6000):
        got, lengths = tok.encode_batch_padded(texts, T, pad_id=1 << 40, truncation=truncation,
                                               padding_side=padding_side)
        want, wlen = _pad_want(ids.astype(np.int64), offsets, T, 1 << 40, truncation, padding_side, np.int64)
        assert np.array_equal(got.cpu().numpy(), want) and lengths.tolist() == wlen.tolist()


def test_padded_many_short_rows():
    import torch
    tok = _byte_tok()
    rng = random.Random(9)
    texts = _texts_with_lengths(tok, [rng.choice((0, 1, 3, 7, 8, 9, 12)) for _ in range(70_000)])
    ids, offsets = tok.encode_batch_np(texts)
    for truncation, padding_side, dtype in (("right", "right", torch.int32), ("left", "left", torch.int64)):
        got, lengths = tok.encode_batch_padded(texts, 8, pad_id=-1, truncation=truncation, padding_side=padding_side,
                                               dtype=dtype)
        want, wlen = _pad_want(ids.astype(np.int64), offsets, 8, -1, truncation, padding_side,
                               np.int32 if dtype == torch.int32 else np.int64)
        assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(lengths.cpu().numpy(), wlen)


def test_pack_rows_argument_errors():
    L = _lib.lib()
    assert L.bpe_ids_pack_rows_device(None, None, 0, 8, 0, 0, 2, None, None, None) == _lib.BPE_E_ARG   # elem_bytes
    assert L.bpe_ids_pack_rows_device(None, None, 0, 8, 0, 4, 4, None, None, None) == _lib.BPE_E_ARG   # flags
    assert L.bpe_ids_pack_rows_device(None, None, 0, 8, 1 << 31, 0, 4, None, None, None) == _lib.BPE_E_ARG
    assert L.bpe_ids_pack_rows_device(None, None, 0, 8, 0, 3, 8, None, None, None) == 0                # no rows


# ---------------------------------------------------------------------- the existing calls
def test_encode_and_encode_file_unchanged(tmp_path):
    """encode(text) and encode_file on a committed golden input give the golden's ids, before and
    after batch calls on the same handle"""
    from bpe_amd.encode import encode_file
    o = G.load("encode", "trained500_corpus_en")
    vocab, merges = G.tokenizer_inputs(o)
    text = G.encode_text(o)
    tok = bpe_amd.Tokenizer(dict(vocab), list(merges), o["special_tokens"])
    assert tok.encode(text) == o["ids"]
    lines = text.splitlines(keepends=True)
    rows = tok.encode_batch(lines)
    assert tok.encode(text) == o["ids"]
    assert rows[:50] == [tok.encode(t) for t in lines[:50]]
    src = tmp_path / "corpus.txt"
    src.write_bytes(text.encode("utf-8"))
    assert "\r" not in text
    assert encode_file(tok, src).tolist() == o["ids"]   # one piece: the text has under 2^20 characters
