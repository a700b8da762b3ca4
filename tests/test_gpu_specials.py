"""GPU: special tokens in Tokenizer.encode (k_find_specials, k_sp_*, the segment handling of
k_enc_scan4 in csrc/encode.hip) and the special filter of training (k_collect_words in
csrc/train_setup.h, k_list_table in csrc/accum.hip), against two references each: the pure-Python
restatement of the reference (oracle.cpu_ref) and the C oracle.  The inputs are those of
tests/special_cases.py; tests/test_special_cases.py shows on the CPU what they reach.

  every case          Tokenizer.encode of every text of every case, both references
  unaligned pointers  bpe_tok_encode_device on a pointer 1, 3, 8 and 15 bytes past a 16-byte
                      boundary (the lead arithmetic of k_find_specials, the unaligned scan): the
                      dense, placement and lengths cases
  piece cuts          bpe_tok_encode_chunks with pieces of 1, 2, 3, 5, 11 and 4099 characters on the
                      overlap and lengths cases, against each piece encoded on its own: cuts inside
                      specials, a shorter prefix taken where the longest is cut
  batch forms         about 40 documents cut at arbitrary characters, inside specials too:
                      encode_batch, encode_batch_np, padded int64 and int32 rows, every document
                      against its own encode and the references
  ranks               2, 3 and 5 in-process ranks on the overlap and context cases: safe split
                      points lie inside "a b" and "b c", the cuts must avoid them
  run-time paths      the joined context case under every knob set of test_gpu_encode.py
  encode_file         pieces of 1000 characters of the dense and many cases, the reference's loop
  special count limit 65 535 specials encode a 300-byte text; 65 536 are BPE_E_LIMIT
  empty special       BPE_E_ARG when the library's tokenizer is built
  training            the lists of special_cases.TRAIN_LISTS (the corpus's own words of 2, 7, 8, 16,
                      17 and 40 bytes, "é", "\\n\\n", "'s", one-byte specials, duplicates, specials
                      that never occur or are no pre-token, early merge products, a list of 70)
                      through train_bpe_bytes, WordCounter.counts and .train (one counter, list
                      after list), train_bpe_word_counts, and two in-process ranks in both modes

Before these tests the library looked each special up in the list of those before it when a
tokenizer was built: with 65 535 specials that loop alone took 6.4 s of host time.  It keeps a set
now (test_special_count_limit: 0.68 s); no test failed for it.  Inputs on which the two references disagree (several equal-length specials missing from
the vocab: the reference numbers them in set order) are kept out of the cases.

Held once against two deliberately wrong builds of the encoder, to see that the cases bite.  One
ignored the ninth byte of a 9-byte special, dropped the matches past the 2048 a workgroup stages
and took a window of 65 segments for one of 64: the lengths, missing, dense and seg_65 tests
failed (35 of the 112 encode tests), seg_64 and seg_many passed.  The other let the byte before a
segment into its clipped window: 94 of the 112 failed.

Measured on an MI355X: the 159 tests take 6.0 s together; the slowest step is the set-up of the
first test, which loads the library (1.5 s); of the tests test_special_count_limit takes 0.68 s,
test_encode[lengths_ascii] 0.29 s (it builds the first tokenizer), test_encode[placement] 0.14 s,
every other 0.13 s or less, reference runs included.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

import special_cases as S
from oracle import cpu_ref, oracle
from test_gpu_encode import RESOLUTION_KNOBS
from test_gpu_encode_batch import _pad_want

pytestmark = pytest.mark.gpu

bpe_amd = pytest.importorskip("bpe_amd")
from bpe_amd import _lib  # noqa: E402

N_DOCS = 40
SHIFTS = (1, 3, 8, 15)
PIECES = (1, 2, 3, 5, 11, 4099)


@pytest.fixture(scope="module", autouse=True)
def _device():
    _lib.require_device()


@functools.lru_cache(maxsize=None)
def _python(name):
    c = S.CASES[name]()
    return cpu_ref.Encoder(c.vocab, c.merges, c.specials)


@functools.lru_cache(maxsize=None)
def _want(name):
    """per text of the case: the ids both references give"""
    c = S.CASES[name]()
    rows = []
    for t in c.texts:
        ids = oracle.encode(c.vocab, c.merges, c.specials, t)
        assert ids == _python(name).encode(t)
        rows.append(ids)
    return rows


def _new_tok(name):
    c = S.CASES[name]()
    return bpe_amd.Tokenizer(dict(c.vocab), list(c.merges), list(c.specials))


@functools.lru_cache(maxsize=None)
def _tok(name):
    return _new_tok(name)


def _same(got, want):
    got, want = list(got), list(want)
    if got != want:
        k = next((j for j, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        pytest.fail(f"{len(got)} ids against {len(want)}, first difference at {k}: {got[k:k + 6]} against {want[k:k + 6]}")


def _family(*families):
    return [n for n, f in S.CASES.items() if f().family in families]


# ---------------------------------------------------------------------- every case
@pytest.mark.parametrize("name", list(S.CASES))
def test_encode(name):
    c, tok = S.CASES[name](), _tok(name)
    for text, want in zip(c.texts, _want(name)):
        _same(tok.encode(text), want)
    if name != "missing":   # (the reference's vocab has no id -> bytes entry for a missing special)
        assert tok.decode(tok.encode(c.text)) == c.text


# ---------------------------------------------------------------------- unaligned pointers
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("name", _family("dense", "placement", "lengths"))
def test_encode_device_unaligned(name, shift):
    import torch
    data = S.CASES[name]().text.encode("utf-8")
    n = len(data)
    buf = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[shift:shift + n] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    out = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    n_out = ctypes.c_size_t(0)
    _lib.check(_lib.lib().bpe_tok_encode_device(_tok(name)._device(), ctypes.c_void_p(buf.data_ptr() + shift), n,
                                                ctypes.c_void_p(out.data_ptr()), ctypes.byref(n_out), None), "encode")
    torch.cuda.synchronize()
    _same(out[:n_out.value].cpu().numpy().view(np.uint32).tolist(), _want(name)[0])


# ---------------------------------------------------------------------- piece cuts
_piece_memo: dict = {}


def _pieces_want(name, k):
    """each piece of k characters encoded on its own: the C oracle in one call over the byte
    offsets, the Python reference piece by piece (a piece met before is not encoded again)"""
    c = S.CASES[name]()
    pieces = [c.text[i:i + k] for i in range(0, len(c.text), k)]
    starts = np.cumsum([0] + [len(p.encode("utf-8")) for p in pieces[:-1]]).astype(np.uint64)
    data = np.frombuffer(c.text.encode("utf-8"), dtype=np.uint8)
    by_oracle = oracle.PieceEncoder(c.vocab, c.merges, c.specials).encode(data.ctypes.data, data.size, starts).tolist()
    memo, enc = _piece_memo.setdefault(name, {}), _python(name)
    by_python = []
    for p in pieces:
        if p not in memo:
            memo[p] = enc.encode(p)
        by_python += memo[p]
    assert by_oracle == by_python
    return starts, by_oracle


@pytest.mark.parametrize("k", PIECES)
@pytest.mark.parametrize("name", _family("overlap", "lengths"))
def test_piece_cuts(name, k):
    starts, want = _pieces_want(name, k)
    data = S.CASES[name]().text.encode("utf-8")
    out = (ctypes.c_uint32 * len(data))()
    n_out = ctypes.c_size_t(0)
    _lib.check(_lib.lib().bpe_tok_encode_chunks(_tok(name)._device(), data, len(data), starts.ctypes.data, len(starts),
                                                out, len(data), ctypes.byref(n_out)), "encode_chunks")
    _same(out[:n_out.value], want)
    if 1 < k < 100:   # the cuts do fall inside specials
        _d, m, lens = S.case_matches(S.CASES[name]())
        cuts = set(starts.tolist())
        assert any(cuts & set(range(p + 1, p + lens[i])) for p, i in m)


# ---------------------------------------------------------------------- batch forms
BATCH = ["overlap", "lengths_utf8", "many", "dense_prefix", "context_joined", "seg_65", "missing"]


@functools.lru_cache(maxsize=None)
def _docs(name):
    return tuple(S.cut_documents(S.CASES[name]().text, N_DOCS, 11))


@functools.lru_cache(maxsize=None)
def _want_docs(name):
    c = S.CASES[name]()
    rows = [oracle.encode(c.vocab, c.merges, c.specials, d) for d in _docs(name)]
    assert rows == [_python(name).encode(d) for d in _docs(name)]
    return rows


@pytest.mark.parametrize("name", BATCH)
def test_encode_batch(name):
    tok, docs, rows = _tok(name), list(_docs(name)), _want_docs(name)
    assert len(docs) == N_DOCS
    assert tok.encode_batch(docs) == rows
    ids, offsets = tok.encode_batch_np(docs)
    assert ids.dtype == np.uint32 and offsets.tolist() == np.cumsum([0] + [len(r) for r in rows]).tolist()
    assert ids.tolist() == [i for r in rows for i in r]
    for d, r in zip(docs, rows):
        assert tok.encode(d) == r


def test_batch_cuts_fall_inside_specials():
    for name in ("overlap", "dense_prefix", "lengths_utf8"):
        c = S.CASES[name]()
        _d, m, lens = S.case_matches(c)
        cuts = set(np.cumsum([len(d.encode("utf-8")) for d in _docs(name)][:-1]).tolist())
        assert any(cuts & set(range(p + 1, p + lens[i])) for p, i in m), name


@pytest.mark.parametrize("dtype", ["int64", "int32"])
@pytest.mark.parametrize("name", BATCH)
def test_encode_batch_padded(name, dtype):
    import torch
    tok, docs, rows = _tok(name), list(_docs(name)), _want_docs(name)
    longest = max(map(len, rows))
    flat = np.array([i for r in rows for i in r], dtype=np.int64)
    offsets = np.cumsum([0] + [len(r) for r in rows])
    tdt = getattr(torch, dtype)
    for T, truncation, padding_side in ((None, "right", "right"), (longest // 2 + 1, "left", "left"),
                                        (longest // 2, "right", "left")):
        got, lengths = tok.encode_batch_padded(docs, T, pad_id=-1, truncation=truncation, padding_side=padding_side,
                                               dtype=tdt)
        want, wlen = _pad_want(flat, offsets, longest if T is None else T, -1, truncation, padding_side, np.dtype(dtype))
        assert got.dtype == tdt and np.array_equal(got.cpu().numpy(), want)
        assert np.array_equal(lengths.cpu().numpy(), wlen)


# ---------------------------------------------------------------------- ranks
@pytest.mark.parametrize("ranks", [2, 3, 5])
@pytest.mark.parametrize("name", _family("overlap", "context"))
def test_encode_several_ranks(name, ranks, monkeypatch):
    """bpe_tok_encode_gpus cuts the text at safe split points no special spans; in the overlap
    text the first candidate at a slab boundary lies inside "a b" or "b c"
    (test_overlap_safe_split_points_inside_specials)"""
    monkeypatch.setenv("BPE355_INPROC_RANKS", "1")
    c, tok = S.CASES[name](), _new_tok(name)
    try:
        bpe_amd.set_num_gpus(ranks)
        got = [tok.encode(t) for t in c.texts]
    finally:
        bpe_amd.set_num_gpus(None)
    for g, want in zip(got, _want(name)):
        _same(g, want)


# ---------------------------------------------------------------------- run-time paths
@pytest.mark.parametrize("knobs", RESOLUTION_KNOBS, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()))
@pytest.mark.parametrize("name", ["context_joined", "seg_65"])
def test_encode_resolution_paths(name, knobs, monkeypatch):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    _same(_new_tok(name).encode(S.CASES[name]().text), _want(name)[0])


# ---------------------------------------------------------------------- encode_file
@pytest.mark.parametrize("name", _family("dense", "many"))
def test_encode_file_pieces(name, tmp_path):
    """encode.py:31-36 with pieces of 1000 characters, as test_encode_file_matches_reference_loop"""
    from bpe_amd.encode import encode_file
    c = S.CASES[name]()
    src = tmp_path / "text.txt"
    src.write_bytes(c.text.encode("utf-8"))
    want, want_python = [], []
    with open(src, "r", encoding="utf-8") as f:
        while True:
            piece = f.read(1000)
            if not piece:
                break
            want += oracle.encode(c.vocab, c.merges, c.specials, piece)
            want_python += _python(name).encode(piece)
    assert want == want_python
    got = encode_file(_tok(name), src, chars_per_piece=1000)
    assert got.dtype == np.uint16
    _same(got.tolist(), want)


# ---------------------------------------------------------------------- limits
def _numbered(n):
    """n specials "<hhhh>", every one a vocab entry after the 256 bytes; a 300-byte text with 20
    of them and near-misses"""
    specials = [f"<{i:04x}>" for i in range(n)]
    vocab = {i: bytes([i]) for i in range(256)}
    for s in specials:
        vocab[len(vocab)] = s.encode()
    text = "".join(f"the <{(i * 7919) % 65535:04x}> cat<12 <{(i * 31) % 65535:04x}" for i in range(20))[:300]
    return specials, vocab, text


def test_special_count_limit():
    """Specials that stand nowhere in the text change nothing in re.split's result, so the
    references run with the ones that do (with all 65 535 each takes 4 to 6 s, in the list
    itself); the vocab is the whole one."""
    specials, vocab, text = _numbered(65535)
    assert len(text.encode()) == 300
    used = [s for s in specials if s in text]
    assert 10 <= len(used) <= 20
    want = oracle.encode(vocab, [], used, text)
    assert want == cpu_ref.Encoder(vocab, [], used).encode(text)
    assert sum(1 for i in want if i >= 256) == len([1 for s in used for _ in range(text.count(s))])
    tok = bpe_amd.Tokenizer(dict(vocab), [], list(specials))
    _same(tok.encode(text), want)
    assert tok.decode(want) == text

    specials, vocab, text = _numbered(65536)
    tok = bpe_amd.Tokenizer(dict(vocab), [], list(specials))
    with pytest.raises(RuntimeError, match=rf"\({_lib.BPE_E_LIMIT}\).*special tokens"):
        tok.encode(text)


def test_empty_special_is_refused():
    vocab = {i: bytes([i]) for i in range(256)}
    tok = bpe_amd.Tokenizer(dict(vocab), [], ["<s>", ""])
    with pytest.raises(RuntimeError, match=rf"\({_lib.BPE_E_ARG}\).*empty special"):
        tok.encode("a<s>b")
    with pytest.raises(RuntimeError, match=rf"\({_lib.BPE_E_ARG}\).*empty special"):
        tok.encode_batch(["a", "b"])


# ---------------------------------------------------------------------- training: the special filter
@functools.lru_cache(maxsize=None)
def _corpus():
    return S.train_corpus().encode("utf-8")


@functools.lru_cache(maxsize=None)
def _train_want(name):
    specials = S.TRAIN_LISTS[name][0]
    vocab, merges, _info = cpu_ref.train(S.train_corpus(), S.TRAIN_VOCAB, specials)
    assert (vocab, merges) == oracle.train_raw(_corpus(), S.TRAIN_VOCAB, specials)
    return vocab, merges


@functools.lru_cache(maxsize=None)
def _words_want(name):
    """the multi-byte pre-tokens that are no special, by both references"""
    specials = S.TRAIN_LISTS[name][0]
    by_python = {w.encode("utf-8"): n for w, n in cpu_ref.count_pretokens(S.train_corpus(), specials).items()}
    by_oracle = oracle.word_counts(_corpus(), specials)
    assert by_python == by_oracle
    return {w: n for w, n in by_oracle.items() if len(w) > 1}


def _same_training(got, name):
    vocab, merges = _train_want(name)
    assert got[1] == merges
    assert got[0] == vocab


@pytest.mark.parametrize("name", list(S.TRAIN_LISTS))
def test_train_bytes(name):
    _same_training(bpe_amd.train_bpe_bytes(_corpus(), S.TRAIN_VOCAB, list(S.TRAIN_LISTS[name][0])), name)


@pytest.fixture(scope="module")
def counter():
    c = bpe_amd.WordCounter().add_bytes(_corpus())
    yield c
    c.close()


@pytest.mark.parametrize("name", list(S.TRAIN_LISTS))
def test_counter_counts_and_train(counter, name):
    """one counter for every list, one after the other"""
    specials = list(S.TRAIN_LISTS[name][0])
    assert counter.counts(specials) == _words_want(name)
    _same_training(counter.train(S.TRAIN_VOCAB, specials), name)


def test_counter_two_lists_in_turn(counter):
    for name in ("words", "long_only", "words", "none", "seventy", "inline_only"):
        specials = list(S.TRAIN_LISTS[name][0])
        _same_training(counter.train(S.TRAIN_VOCAB, specials), name)
        assert counter.counts(specials) == _words_want(name)


@pytest.mark.parametrize("name", list(S.TRAIN_LISTS))
def test_train_word_counts(name):
    """the unfiltered counts of the corpus (str keys, one-byte words included) and the list"""
    counts = cpu_ref.count_pretokens(S.train_corpus(), [])
    _same_training(bpe_amd.train_bpe_word_counts(counts, S.TRAIN_VOCAB, list(S.TRAIN_LISTS[name][0])), name)


@pytest.fixture
def ranks(monkeypatch):
    def set_(n, mode):
        monkeypatch.setenv("BPE355_INPROC_RANKS", "1")
        monkeypatch.setenv("BPE355_EXCHANGE", mode)
        bpe_amd.set_num_gpus(n)
    yield set_
    bpe_amd.set_num_gpus(None)


@pytest.mark.parametrize("mode", ["words", "rounds"])
@pytest.mark.parametrize("name", ["words", "one_byte", "duplicates", "merge_products", "seventy"])
def test_train_two_ranks(name, mode, ranks):
    ranks(2, mode)
    got = bpe_amd.train_bpe_bytes(_corpus(), S.TRAIN_VOCAB, list(S.TRAIN_LISTS[name][0]))
    assert bpe_amd.last_train_stats()["n_gpus"] == 2
    _same_training(got, name)
