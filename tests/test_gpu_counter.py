"""WordCounter (csrc/accum.hip, the window driver in csrc/drive.hip) against the oracle's Counter
(reference train.py:16-49 over a corpus fed document by document) and oracle.train_raw: document
boundaries, shards in either order, one shard against today's path and the goldens, the three key
paths with words shared between shards and not, table and pool growth from tiny sizes, files
counted window by window (LF, CRLF, a run without a safe split point), errors that leave the
counter unchanged, words in and out, repeated training with different vocab sizes and specials,
and the tie-heavy cases cut into two documents."""
from __future__ import annotations

import struct

import numpy as np
import pytest

import golden_cases as G
import synth_text
import tie_cases
from oracle import oracle

pytestmark = pytest.mark.gpu

bpe_amd = pytest.importorskip("bpe_amd")
from bpe_amd import _lib  # noqa: E402
from bpe_amd.train import last_train_stats  # noqa: E402

EOT = ["<|endoftext|>"]


@pytest.fixture
def knob(monkeypatch):
    def set_(k, v):
        monkeypatch.setenv(k, str(v))
    return set_


def _synth(seed, flavour, n):
    buf = np.empty(n, dtype=np.uint8)
    assert _lib.lib().bpe_synth_corpus_host(buf.ctypes.data, n, seed, flavour, 0, 8) == 0
    return buf.tobytes()


def _oracle_counter(docs, specials=()):
    c = oracle.Counter(specials)
    for d in docs:
        if d:
            a = np.frombuffer(d, dtype=np.uint8)
            c.feed(a.ctypes.data, len(d))
    return c


def _oracle_words(docs, specials=()):
    return {w: n for w, n in _oracle_counter(docs, specials).words().items() if len(w) > 1}


def _counter(docs):
    c = bpe_amd.WordCounter()
    for d in docs:
        c.add_bytes(d)
    return c


def _translated(data):
    return data.replace(b"\r\n", b"\n").replace(b"\r", b"\n")


# ---------------------------------------------------------------- 1. document boundaries
def test_document_boundaries():
    docs = [b"hello wor", b"ld peace"]
    c = _counter(docs)
    got = c.counts()
    assert got == _oracle_words(docs)
    assert got[b" wor"] == 1 and got[b"ld"] == 1 and b" world" not in got
    whole = _counter([b"".join(docs)]).counts()
    assert whole != got and whole[b" world"] == 1
    assert c.info()["n_inputs"] == 2


# ---------------------------------------------------------------- 2. sharded training
@pytest.fixture(scope="module")
def shards():
    docs = [_synth(41, 0, 3 << 20), _synth(42, 1, 2 << 20),
            synth_text.generate(43, 2_000_000, "mixed").encode("utf-8")]
    assert all((2 << 20) <= len(d) <= (4 << 20) for d in docs), [len(d) for d in docs]
    return docs, _oracle_counter(docs, EOT).train(2000)


@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_sharded_training(shards, order):
    docs, want = shards
    c = _counter(docs if order == "forward" else docs[::-1])
    assert c.train(2000, EOT) == want
    st = last_train_stats()
    assert st["n_bytes"] == sum(len(_translated(d)) for d in docs)
    assert st["n_pretokens"] == c.info()["n_pretokens"] > 0
    assert st["n_words"] == len(c.counts(EOT))


# ---------------------------------------------------------------- 3. one shard equals today's path
@pytest.mark.parametrize("name", G.names("train"))
def test_one_shard_equals_train_bpe_and_golden(name):
    o, vocab, merges = G.train_expect(name)
    data = G.input_bytes(o["input"])
    c = bpe_amd.WordCounter().add_bytes(data)
    got = c.train(o["vocab_size"], o["special_tokens"])
    assert got == bpe_amd.train_bpe_bytes(data, o["vocab_size"], o["special_tokens"])
    assert got == (vocab, merges)


# ---------------------------------------------------------------- 4. key paths and duplicates
LENGTHS = (2, 7, 8, 16, 17, 64, 5000)


def _word(length, tag):
    """a pre-token of `length` bytes: a space and length - 1 letters, distinct per (length, tag)"""
    body = (tag * length)[:length - 2] + "qjz"[LENGTHS.index(length) % 3] if length > 2 else tag[0]
    return (" " + body)[:length]


def test_key_paths_and_duplicates():
    both = {L: _word(L, "ab") for L in LENGTHS}
    only1 = {L: _word(L, "cd") for L in LENGTHS}
    only2 = {L: _word(L, "ef") for L in LENGTHS}
    assert all(len(w[L]) == L for w in (both, only1, only2) for L in LENGTHS)
    assert len({w[L] for w in (both, only1, only2) for L in LENGTHS}) == 3 * len(LENGTHS)
    d1 = ("zz" + "".join(both[L] * (i + 2) + only1[L] * (i + 1) for i, L in enumerate(LENGTHS))).encode()
    d2 = ("zz" + "".join(only2[L] * (i + 3) + both[L] * (i + 5) for i, L in enumerate(LENGTHS))).encode()
    c = _counter([d1, d2])
    got = c.counts()
    assert got == _oracle_words([d1, d2])
    for i, L in enumerate(LENGTHS):
        assert got[both[L].encode()] == (i + 2) + (i + 5)
        assert got[only1[L].encode()] == i + 1
        assert got[only2[L].encode()] == i + 3
    assert c.train(400, []) == _oracle_counter([d1, d2]).train(400)


# ---------------------------------------------------------------- 5. growth at small sizes
def test_growth_from_tiny_table_and_pool(knob):
    data = _synth(44, 0, 2 << 20)
    docs = [data[i:i + (512 << 10)] for i in range(0, len(data), 512 << 10)]   # whole 4096-byte blocks
    want = _oracle_words(docs)
    plain = _counter(docs)
    knob("BPE355_ACC_SLOTS", 64)
    knob("BPE355_ACC_POOL", 256)
    c = bpe_amd.WordCounter()
    assert c.info()["table_slots"] == 64 and c.info()["pool_bytes"] == 256
    for d in docs:
        c.add_bytes(d)
    info = c.info()
    assert info["n_grows"] > 1
    assert info["n_words"] == len(want) and 2 * info["n_words"] <= info["table_slots"]
    assert info["pool_live_bytes"] == sum(len(w) for w in want) <= info["pool_bytes"]
    assert c.counts() == want == plain.counts()
    assert c.train(1500, EOT) == plain.train(1500, EOT) == _oracle_counter(docs, EOT).train(1500)


# ---------------------------------------------------------------- 6. windows
def _file_cases():
    base = _synth(45, 0, 3 << 20)
    run = b"".join(b"w%d\n" % (i % 977) for i in range(70_000))[:300_000]   # no U+0020: no safe split point
    assert b" " not in run and len(run) == 300_000
    crlf = base.replace(b"\n", b"\r\n")
    assert crlf.count(b"\r\n") > 100
    return {"lf": base, "crlf": crlf, "run": base[:1 << 20] + b"\n" + run + base[1 << 20:2 << 20]}


@pytest.fixture(scope="module")
def file_cases(tmp_path_factory):
    d = tmp_path_factory.mktemp("counter_files")
    out = {}
    for name, data in _file_cases().items():
        p = d / f"{name}.txt"
        p.write_bytes(data)
        out[name] = (p, data, bpe_amd.train_bpe(p, 1200, EOT), _oracle_words([data], EOT))
    return out


@pytest.mark.parametrize("window", [64 << 10, 1 << 20])
@pytest.mark.parametrize("case", ["lf", "crlf", "run"])
def test_windows(file_cases, case, window):
    p, data, want_train, want_words = file_cases[case]
    c = bpe_amd.WordCounter().add_file(p, window)
    info = c.info()
    assert info["n_windows"] > 1 and info["n_inputs"] == 1
    if case == "run" and window < 300_000:
        assert info["max_window_bytes"] >= 300_000   # the window ran on to the next safe point
    else:
        assert info["max_window_bytes"] <= 2 * window
    assert info["n_bytes"] == len(_translated(data))
    assert c.counts(EOT) == want_words
    assert c.train(1200, EOT) == want_train
    assert bpe_amd.train_bpe_files([p], 1200, EOT, window_bytes=window) == want_train


# ---------------------------------------------------------------- 7. errors
def test_errors_leave_the_counter_unchanged(tmp_path):
    data = bytearray(_synth(46, 0, 256 << 10))
    data[150_000] = 0xFF
    p = tmp_path / "bad.txt"
    p.write_bytes(bytes(data))
    with pytest.raises(UnicodeDecodeError) as want:
        bpe_amd.train_bpe(p, 300, [])
    assert 150_000 - 4 < want.value.start <= 150_000   # (a multi-byte character may begin just before it)
    c = _counter([b"hello world hello world"])
    before = c.counts()
    info = c.info()
    with pytest.raises(UnicodeDecodeError) as e:
        c.add_file(p, 128 << 10)   # the bad byte lies in the second window
    assert (e.value.start, e.value.end) == (want.value.start, want.value.end)
    with pytest.raises(FileNotFoundError):
        c.add_file(tmp_path / "missing.txt")
    blob = struct.pack("<I", 3) + b" ab" + struct.pack("<Q", 4) + struct.pack("<I", 5) + b" cd"
    with pytest.raises(ValueError):
        c.add_words_blob(blob)
    with pytest.raises(ValueError):
        c.add_words_blob(blob[:13])
    assert c.counts() == before and c.info() == info
    with pytest.raises(FileNotFoundError):
        bpe_amd.train_bpe_files([tmp_path / "missing.txt"], 300, [])


# ---------------------------------------------------------------- 8. words in and out
def test_words_in_and_out():
    sp = [" the"] + EOT
    data = G.input_bytes({"kind": "fixture", "name": "corpus.en"})
    text = _translated(data)
    assert bpe_amd.train_bpe_word_counts(oracle.word_counts(text, sp), 800, sp) == oracle.train_raw(data, 800, sp)
    cut = _lib.lib().bpe_safe_split(data, len(data), 60_000)
    assert cut
    a, b = data[:cut], data[cut:]
    c = _counter([a, b])
    again = bpe_amd.WordCounter().add_counts(c.counts())
    assert again.counts() == c.counts() == _oracle_words([a, b])
    assert again.info()["n_pretokens"] == c.info()["n_pretokens"]
    str_keys = bpe_amd.WordCounter().add_counts({"é": 3, " ab": 2, "x": 9, " zero": 0}).add_counts({b" ab": 5})
    assert str_keys.counts() == {"é".encode(): 3, b" ab": 7}
    u = _counter([a]).absorb(_counter([b]))
    assert u.counts() == c.counts()
    assert u.train(700, EOT) == c.train(700, EOT) == _oracle_counter([a, b], EOT).train(700)


# ---------------------------------------------------------------- 9. not consumed; specials at train time
def test_not_consumed_and_specials_at_train_time():
    docs = [_synth(47, 1, 1 << 20), G.input_bytes({"kind": "fixture", "name": "corpus.en"}), _synth(49, 0, 1 << 20)]
    c = _counter(docs[:2])
    _v6, m600 = c.train(600, EOT)
    _v9, m900 = c.train(900, EOT)
    assert len(m600) == 600 - 257 and m900[:len(m600)] == m600
    assert (_v9, m900) == _oracle_counter(docs[:2], EOT).train(900)
    c.add_bytes(docs[2])
    assert c.train(900, EOT) == _oracle_counter(docs, EOT).train(900)
    for sp in ([], [" the"]):
        assert c.counts(sp) == _oracle_words(docs, sp)
        assert c.train(700, sp) == _oracle_counter(docs, sp).train(700)
    assert b" the" in c.counts([]) and b" the" not in c.counts([" the"])


# ---------------------------------------------------------------- 10. tie-heavy
@pytest.mark.parametrize("kind,seed", tie_cases.all_cases())
def test_tie_cases_in_two_documents(kind, seed):
    data = tie_cases.case(seed, kind).encode("utf-8")
    cut = _lib.lib().bpe_safe_split(data, len(data), len(data) // 2)
    if not cut:   # ("nulstem" separates its words by newlines: cut behind one)
        cut = data.index(b"\n", len(data) // 2) + 1
    docs = [data[:cut], data[cut:]]
    assert all(docs)
    c = _counter(docs)
    assert c.counts() == _oracle_words(docs)
    assert c.train(tie_cases.VOCAB, []) == _oracle_counter(docs).train(tie_cases.VOCAB)


# ---------------------------------------------------------------- the other inputs
def test_tensor_text_and_clear():
    import torch
    data = synth_text.generate(50, 200_000, "mixed").encode("utf-8")
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    c = bpe_amd.WordCounter().add_tensor(t)
    want = _oracle_words([data])
    assert c.counts() == want
    assert bytes(t.cpu().numpy()) == data
    c.add_text(data.decode("utf-8"))
    assert c.counts() == {w: 2 * n for w, n in want.items()}
    c.clear()
    assert c.counts() == {} and c.info()["n_words"] == 0 and c.info()["n_pretokens"] == 0
    c.add_bytes(data)
    assert c.counts() == want
    c.close()
    with pytest.raises(ValueError):
        c.counts()
