"""GPU: training parity at the word-length edges of the merge loop (csrc/train.hip), bit-exact
against the C oracle: ordered merges and the id -> bytes vocab.  The texts are those of
tests/word_length_cases.py; tests/test_word_length_cases.py shows on the CPU that they hold words
on both sides of every slot-class boundary (7|8, 15|16, 31|32, 63|64 ids) and far past the last,
that every class and the long table are rewritten (several occurrences per word among them), that
words move down through every class, that the token pool must grow and that "runs" and "periodic"
run out of pairs early.

  parity matrix     every kind at vocab 300 (no compaction inside the loop), 1500 (compactions,
                    pool growth, class migration) and 66 000 (the uint32_t instantiation, to
                    exhaustion), on the batched trips, the per-round kernels (BPE355_BATCH=0), one
                    member per trip, the fused trip, the 64-bit global cells and the touched-block
                    marks from 128 tokens on with their check
  u16 | u32         vocab 65 533 is the last that trains on uint16_t ids, 65 534 the first on
                    uint32_t (train_text: 256 + rounds + 1 < 65535)
  single lengths    three words of one length: one class, or only the long table, is occupied
  many long words   more long words than the 64 * 256 threads of the long-word blocks; list
                    rounds and full scans both occur
  not vacuous       the device's own counters and its traced class layouts
  several ranks     in-process ranks, both word exchanges and the per-round all-reduce
  round trip        the device-trained tokenizer encodes and decodes its own training text

The runs at vocab 65 533 and above go on until no pair is left; for "random" they train on
W.to_exhaustion's text, which keeps one word at each length from 1000 on (see there).

Measured on an MI355X: the 171 tests take 92 s together, oracle included.  The slowest are the twelve
that take a random word of 4097 ids down to one token: test_single_length[4097-66000-*] 6.1-6.2 s,
test_parity_matrix[random-66000-*] and test_u16_u32_switch 5.7-5.9 s, the other seeds 4.0-4.6 s;
every other test takes 1.9 s or less.  That time is the device's: the long-word blocks give each
long word to one thread, which reads what is left of it id by id in every trip (1.7 ms per round
for three words of 4097 ids against 42 us for three of 66), and a word of random letters needs
thousands of rounds of its own.  With three such words of different counts ("random" whole) the
same run took 16.5 s, so the text was cut to one; the word itself cannot be shorter than the
length list asks.
"""
from __future__ import annotations

import functools
import re
import struct

import pytest

import word_length_cases as W
from oracle import oracle

pytestmark = pytest.mark.gpu

bpe_amd = pytest.importorskip("bpe_amd")

# knobs the library reads on every call (as test_gpu_train.py's test_train_runtime_variants)
KNOBS = [None, "BPE355_BATCH=0", "BPE355_BATCH=1", "BPE355_FOLD=1", "BPE355_LDS_CELLS=0",
         "BPE355_DENSE_TOK=128+BPE355_SPARSE_FROM=128+BPE355_CHECK_MARKS=1"]


@pytest.fixture(scope="module", autouse=True)
def _device():
    from bpe_amd import _lib
    _lib.require_device()


@pytest.fixture
def ranks(monkeypatch):
    def set_(n, mode):
        monkeypatch.setenv("BPE355_INPROC_RANKS", "1")
        if mode == "words-gather":
            monkeypatch.setenv("BPE355_EXCHANGE_OWNER", "0")
            mode = "words"
        monkeypatch.setenv("BPE355_EXCHANGE", mode)
        bpe_amd.set_num_gpus(n)
    yield set_
    bpe_amd.set_num_gpus(None)


@functools.lru_cache(maxsize=None)
def _data(kind, seed, vocab=1500):
    """(from vocab 65 533 on every run goes on until no pair is left: W.to_exhaustion)"""
    return (W.to_exhaustion(kind, seed) if vocab > 60000 else W.case(kind, seed)).encode("utf-8")


@functools.lru_cache(maxsize=None)
def _want(kind, seed, vocab):
    return oracle.train_raw(_data(kind, seed, vocab), vocab, [])


def _set(knob, monkeypatch):
    for kv in (knob or "").split("+"):
        if kv:
            monkeypatch.setenv(*kv.split("="))


def _check(got, want):
    g_vocab, g_merges = got
    w_vocab, w_merges = want
    if g_merges != w_merges:
        i = next((k for k, (a, b) in enumerate(zip(g_merges, w_merges)) if a != b),
                 min(len(g_merges), len(w_merges)))
        pytest.fail(f"merges differ at round {i} of {len(g_merges)} / {len(w_merges)}: device "
                    f"{[(a[:24], len(a), b[:24], len(b)) for a, b in g_merges[i:i + 2]]!r}, oracle "
                    f"{[(a[:24], len(a), b[:24], len(b)) for a, b in w_merges[i:i + 2]]!r}")
    assert g_vocab == w_vocab


@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("vocab", W.VOCABS)
@pytest.mark.parametrize("kind", W.KINDS)
def test_parity_matrix(kind, vocab, knob, monkeypatch):
    _set(knob, monkeypatch)
    _check(bpe_amd.train_bpe_bytes(_data(kind, 0, vocab), vocab, []), _want(kind, 0, vocab))


@pytest.mark.parametrize("vocab", W.VOCABS)
@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("kind", W.KINDS)
def test_parity_other_seeds(kind, seed, vocab):
    _check(bpe_amd.train_bpe_bytes(_data(kind, seed, vocab), vocab, []), _want(kind, seed, vocab))


_switch_got = {}


@pytest.mark.parametrize("vocab", [65533, 65534])
def test_u16_u32_switch(vocab):
    """vocab 65 533: 256 + 65 277 + 1 = 65 534 < 65 535, uint16_t ids; vocab 65 534: uint32_t."""
    got = bpe_amd.train_bpe_bytes(_data("random", 0, vocab), vocab, [])
    _switch_got[vocab] = got
    _check(got, _want("random", 0, vocab))
    assert len(got[1]) > 1500


def test_u16_u32_switch_same_merges():
    """The two runs above against each other, up to where the shorter stops."""
    if len(_switch_got) < 2:    # (run alone: make them here)
        for vocab in (65533, 65534):
            _switch_got[vocab] = bpe_amd.train_bpe_bytes(_data("random", 0, vocab), vocab, [])
    got16, got32 = _switch_got[65533], _switch_got[65534]
    n = min(len(got16[1]), len(got32[1]))
    assert n > 1500 and got16[1][:n] == got32[1][:n]
    assert all(got16[0][i] == got32[0][i] for i in range(min(len(got16[0]), len(got32[0]))))


@pytest.mark.parametrize("knob", [None, "BPE355_BATCH=0"])
@pytest.mark.parametrize("vocab", [300, 66000])
@pytest.mark.parametrize("L", W.LENGTHS)
def test_single_length(L, vocab, knob, monkeypatch):
    _set(knob, monkeypatch)
    data = W.single_length_case(L).encode("utf-8")
    _check(bpe_amd.train_bpe_bytes(data, vocab, []), oracle.train_raw(data, vocab, []))


@functools.lru_cache(maxsize=None)
def _many_long():
    data = W.many_long_case().encode("utf-8")
    return data, oracle.train_raw(data, W.MANY_LONG_VOCAB, [])


def test_many_long_words():
    data, want = _many_long()
    _check(bpe_amd.train_bpe_bytes(data, W.MANY_LONG_VOCAB, []), want)


def test_many_long_words_per_round(tmp_path, monkeypatch):
    """The per-round kernels, with their round log: 24-byte records {a, b, new, list length
    (0xffffffff: a full scan), count}.  Measured on an MI355X: 1209 list rounds and 535 full scans
    of the 1744."""
    data, want = _many_long()
    log = tmp_path / "rounds.bin"
    monkeypatch.setenv("BPE355_BATCH", "0")
    monkeypatch.setenv("BPE355_ROUND_LOG", str(log))
    _check(bpe_amd.train_bpe_bytes(data, W.MANY_LONG_VOCAB, []), want)
    raw = log.read_bytes()
    recs = [struct.unpack_from("<IIIIq", raw, o) for o in range(0, len(raw), 24)]
    assert len(recs) == len(want[1])
    full = sum(r[3] == 0xFFFFFFFF for r in recs)
    print(f"many long words: {len(recs) - full} list rounds, {full} full scans")
    assert full >= 1 and len(recs) - full >= 1


def test_device_counters_not_vacuous():
    """n_trips counts the trips that made a merge, n_rounds_batched only the rounds of trips that
    made more than one (MergeLoop::finish_block), so "some trip took more than one merge" is
    rounds > trips, with every round made on the device."""
    got = bpe_amd.train_bpe_bytes(_data("random", 0), 1500, [])
    _check(got, _want("random", 0, 1500))
    st = bpe_amd.last_train_stats()
    print({k: st[k] for k in ("n_index_builds", "n_trips", "n_rounds_batched", "n_rounds_device")})
    assert st["n_index_builds"] >= 2              # a compaction ran inside the loop
    assert st["n_rounds_device"] == len(got[1]) == 1500 - 256
    assert st["n_rounds_device"] > st["n_trips"] > 0   # some trip took more than one merge
    assert st["n_rounds_batched"] >= 2


def test_traced_class_layouts(monkeypatch, capfd):
    """(The one test that reads layout_blocks' trace line.)"""
    monkeypatch.setenv("BPE355_TRACE", "1")
    got = bpe_amd.train_bpe_bytes(_data("random", 0), 1500, [])
    err = capfd.readouterr().err
    _check(got, _want("random", 0, 1500))
    layouts = [tuple(map(int, m.groups())) for m in
               re.finditer(r"words per slot class: (\d+) (\d+) (\d+) (\d+), long (\d+)", err)]
    print(layouts)
    assert len(layouts) >= 2
    assert any(all(x > 0 for x in lay) for lay in layouts)   # every class and the long table in use
    assert layouts[-1][4] < layouts[0][4]                    # long words shrank into the slots


@pytest.mark.parametrize("mode,n", [("words", 3), ("words-gather", 2), ("rounds", 2)])
def test_several_ranks(mode, n, ranks):
    """Slabs cut at safe points around the 4 KB pre-tokens; the word exchange carries words keyed
    by an occurrence; "rounds" runs k_merge's long-word branch on every rank."""
    ranks(n, mode)
    got = bpe_amd.train_bpe_bytes(_data("random", 0), 1500, [])
    assert bpe_amd.last_train_stats()["n_gpus"] == n
    _check(got, _want("random", 0, 1500))


def test_round_trip():
    """Tokens of up to ~3000 bytes: outside the encoder's dictionary of 2-16 byte tokens."""
    text = W.case("random", 0)
    vocab, merges = bpe_amd.train_bpe_bytes(_data("random", 0), 1500, [])
    _check((vocab, merges), _want("random", 0, 1500))
    assert max(map(len, vocab.values())) > 1000
    tok = bpe_amd.Tokenizer(dict(vocab), list(merges), [])
    try:
        ids = tok.encode(text)
        assert ids == oracle.encode(vocab, merges, [], text)
        assert tok.decode(ids) == text
    finally:
        tok.release_device_buffers()
