"""GPU: training on word counts from 2^31 up to the documented limit (the sum of count * length
below 2^62), bit-exact against tests/big_count_cases.py's train_counts: ordered merges and the
id -> bytes vocab, and through the round log every round's winning count.  No text reaches such
counts; WordCounter.add_counts does.  tests/test_big_count_cases.py shows on the CPU that the
cases are what they claim and that train_counts is the reference trainer.

  parity            every case on the batched trips, the per-round kernels (BPE355_BATCH=0), one
                    member per trip, the fused trip, the 64-bit global cells and the touched-block
                    marks from 128 tokens on with their check; boundary(V) also to exhaustion on
                    uint32_t ids; a run of 2044 rounds whose first pair table of 2^18 slots must
                    grow (k_rehash)
  round counts      the device's own count of each round's winner (BPE355_ROUND_LOG) equals the
                    reference's: a counter off by a multiple of 2^32 that kept the order shows here
  not vacuous       crossing's logged counts lie on both sides of 2^32 and 2^31; compactions and
                    multi-merge trips ran at these magnitudes
  the accumulator   sums that pass 2^32 in add_counts, absorb and within one blob, for the three
                    key layouts; n_pretokens exact; words out and in again
  the limit         weight 2^62 - 2 is accepted and trains; 2^62 and products that overflow 64 bits
                    are refused with the limit error and change nothing, also when only the sum
                    of two calls, or an absorb, passes it

The reference of each case is computed once (functools.lru_cache) and shared by every variant.

Measured on an MI355X: the 241 tests take 13 s together, every reference included.  The slowest is
test_parity[near_limit-None] at 2.1 s, nearly all of it that case's reference in plain Python (its
counts take three machine words each), computed there once; the first test of the module waits
1.9 s for the device; the first use of each other case built on "synth" takes 0.5-0.8 s, the growth
test 0.3 s, every other test 0.17 s or less.
"""
from __future__ import annotations

import functools
import re
import struct

import pytest

import big_count_cases as B

pytestmark = pytest.mark.gpu

bpe_amd = pytest.importorskip("bpe_amd")
from bpe_amd.train import last_train_stats  # noqa: E402

# knobs the library reads on every call (as test_gpu_word_lengths.py)
KNOBS = [None, "BPE355_BATCH=0", "BPE355_BATCH=1", "BPE355_FOLD=1", "BPE355_LDS_CELLS=0",
         "BPE355_DENSE_TOK=128+BPE355_SPARSE_FROM=128+BPE355_CHECK_MARKS=1"]
CASES = B.parity_cases()
LOGGED = ["crossing", "near_limit"] + [c for c in CASES if c.startswith(("boundary", "one_block"))]
LIMIT_ERROR = r"\(-8\).*pair counters"


@pytest.fixture(scope="module", autouse=True)
def _device():
    from bpe_amd import _lib
    _lib.require_device()


@functools.lru_cache(maxsize=None)
def _counts(case):
    return CASES[case][0]()


@functools.lru_cache(maxsize=None)
def _want(case):
    """(vocab, merges, each round's best count) of the reference."""
    _build, vocab, specials = CASES[case]
    return B.tops(_counts(case), vocab, specials)


@functools.lru_cache(maxsize=None)
def _exhaust(V):
    counts = B.boundary(V, B.EXHAUST_WORDS)
    return counts, B.tops(counts, B.EXHAUST_VOCAB)


def _set(knob, monkeypatch):
    for kv in (knob or "").split("+"):
        if kv:
            monkeypatch.setenv(*kv.split("="))


def _check(got, want):
    g_vocab, g_merges = got
    w_vocab, w_merges = want[0], want[1]
    if g_merges != w_merges:
        i = next((k for k, (a, b) in enumerate(zip(g_merges, w_merges)) if a != b),
                 min(len(g_merges), len(w_merges)))
        pytest.fail(f"merges differ at round {i} of {len(g_merges)} / {len(w_merges)}: device "
                    f"{g_merges[i:i + 2]!r}, reference {w_merges[i:i + 2]!r}")
    assert g_vocab == w_vocab


def _train(case):
    _build, vocab, specials = CASES[case]
    return bpe_amd.train_bpe_word_counts(_counts(case), vocab, list(specials))


def _logged_counts(path):
    """The round log's 24-byte records {a, b, new, list length, count}: the counts."""
    raw = path.read_bytes()
    assert len(raw) % 24 == 0
    return [struct.unpack_from("<IIIIq", raw, o)[4] for o in range(0, len(raw), 24)]


# ---------------------------------------------------------------- parity
@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("case", list(CASES))
def test_parity(case, knob, monkeypatch):
    _set(knob, monkeypatch)
    _check(_train(case), _want(case))


@pytest.mark.parametrize("V", B.BOUNDARY_VS)
def test_boundary_to_exhaustion_u32(V):
    """vocab 66 000: k_merge_batch<uint32_t> and the u32 word tables, until no pair is left."""
    counts, want = _exhaust(V)
    got = bpe_amd.train_bpe_word_counts(counts, B.EXHAUST_VOCAB, [])
    _check(got, want)
    assert 300 < len(got[1]) < B.EXHAUST_VOCAB - 256


def test_crossing_small_pair_table(monkeypatch):
    """(The smallest first table; crossing's 1200 tokens do not make it grow: the next test does.)"""
    monkeypatch.setenv("BPE355_PAIR_CAP_LOG2", "18")
    _check(_train("crossing"), _want("crossing"))


def test_pair_table_grows(tmp_path, monkeypatch, capfd):
    """grow_pairs / k_rehash move counts that are all multiples of 2^33 - 1 (B.grows_pair_table).
    That the table grew is read from the trace's host clock line (its time in grow_pairs).  By then
    most live counts are the factor itself, tied: counts cut to 32 bits by the rehash would keep
    these merges, and show in the logged counts of the rounds after it."""
    log = tmp_path / "rounds.bin"
    monkeypatch.setenv("BPE355_ROUND_LOG", str(log))
    monkeypatch.setenv("BPE355_PAIR_CAP_LOG2", "18")
    monkeypatch.setenv("BPE355_TRACE", "1")
    counts = B.grows_pair_table()
    got = bpe_amd.train_bpe_word_counts(counts, B.GROW_VOCAB, [])
    err = capfd.readouterr().err
    want = B.tops(counts, B.GROW_VOCAB)
    _check(got, want)
    assert _logged_counts(log) == want[2]
    grow_ms = [float(m.group(1))
               for m in re.finditer(r"merge loop host clock: rebuild [\d.]+ ms, grow ([\d.]+),", err)]
    print(f"pair table growth: {grow_ms} ms")
    assert grow_ms and grow_ms[0] > 0


# ---------------------------------------------------------------- the counters themselves
@pytest.mark.parametrize("knob", [None, "BPE355_BATCH=0"])
@pytest.mark.parametrize("case", LOGGED)
def test_round_counts(case, knob, tmp_path, monkeypatch):
    _set(knob, monkeypatch)
    log = tmp_path / "rounds.bin"
    monkeypatch.setenv("BPE355_ROUND_LOG", str(log))
    want = _want(case)
    _check(_train(case), want)
    got = _logged_counts(log)
    assert len(got) == len(want[2])
    bad = [(r, g, w) for r, (g, w) in enumerate(zip(got, want[2])) if g != w]
    assert not bad, f"{len(bad)} rounds with another count; the first (round, device, reference): {bad[:3]}"


def test_not_vacuous_on_the_device(tmp_path, monkeypatch):
    log = tmp_path / "rounds.bin"
    monkeypatch.setenv("BPE355_ROUND_LOG", str(log))
    got = _train("crossing")
    _check(got, _want("crossing"))
    st = last_train_stats()
    counts = _logged_counts(log)
    high, low = sum(c >= 1 << 32 for c in counts), sum(c < 1 << 31 for c in counts)
    print(f"crossing: {high} logged rounds at 2^32 or above, {low} below 2^31;",
          {k: st[k] for k in ("n_index_builds", "n_trips", "n_rounds_batched", "n_rounds_device")})
    assert high >= 100 and low >= 100
    assert st["n_index_builds"] >= 2                     # a compaction ran inside the loop
    assert st["n_rounds_device"] == len(got[1])
    assert st["n_rounds_device"] > st["n_trips"] > 0     # some trip took more than one merge


# ---------------------------------------------------------------- the accumulator
def _word(n):
    """n bytes: the inline key (<= 7), the packed compare (8-16), words_equal (> 16)"""
    return (" " + "abcdefghij" * 7)[:n].encode()


KEY_LENGTHS = (2, 7, 8, 16, 17, 70)


@pytest.mark.parametrize("n", KEY_LENGTHS)
def test_sums_pass_2_32(n):
    w, other = _word(n), _word(n)[:-1] + b"z"
    c = bpe_amd.WordCounter().add_counts({w: (1 << 32) - 1, other: 7})
    assert c.counts() == {w: (1 << 32) - 1, other: 7}
    c.add_counts({w: 1})                                  # the fold's atomic add onto the word
    assert c.counts() == {w: 1 << 32, other: 7}
    c.add_counts({w: (1 << 32) - 1})
    assert c.counts() == {w: (1 << 33) - 1, other: 7}
    assert c.info()["n_words"] == 2 and c.info()["n_pretokens"] == (1 << 33) - 1 + 7

    a = bpe_amd.WordCounter().add_counts({w: (1 << 32) - 1})
    a.absorb(bpe_amd.WordCounter().add_counts({w: 1, other: 7}))
    assert a.counts() == {w: 1 << 32, other: 7}
    a.absorb(bpe_amd.WordCounter().add_counts({w: (1 << 32) - 1}))
    assert a.counts() == c.counts() and a.info()["n_pretokens"] == c.info()["n_pretokens"]


@pytest.mark.parametrize("n", KEY_LENGTHS)
def test_one_blob_with_the_word_twice(n):
    """add_records merges equal words on the host before the upload."""
    w = _word(n)
    rec = lambda c: struct.pack("<I", len(w)) + w + struct.pack("<Q", c)   # noqa: E731
    c = bpe_amd.WordCounter().add_words_blob(rec((1 << 32) - 1) + rec(2) + rec(1 << 40))
    assert c.counts() == {w: (1 << 40) + (1 << 32) + 1}
    assert c.info()["n_pretokens"] == (1 << 40) + (1 << 32) + 1


def test_pretoken_sums_and_words_out_and_in():
    counts = _counts("scaled-synth-0x1ffffffff")
    kept = {w: n for w, n in counts.items() if len(w) >= 2}
    total = B.n_pretokens(counts)
    assert total == sum(kept.values()) >= len(kept) * ((1 << 33) - 1) > 1 << 45
    c = bpe_amd.WordCounter().add_counts(counts)
    assert c.counts() == kept
    assert c.info()["n_pretokens"] == total
    want = _want("scaled-synth-0x100000000")              # (the same text: the same merges)
    _check(c.train(B.VOCAB, []), want)
    assert last_train_stats()["n_pretokens"] == total
    again = bpe_amd.WordCounter().add_counts(c.counts())
    assert again.counts() == kept and again.info()["n_pretokens"] == total
    _check(again.train(B.VOCAB, []), want)
    assert last_train_stats()["n_pretokens"] == total


# ---------------------------------------------------------------- the limit
def test_weight_just_below_the_limit(tmp_path, monkeypatch):
    log = tmp_path / "rounds.bin"
    monkeypatch.setenv("BPE355_ROUND_LOG", str(log))
    n = (1 << 61) - 1
    assert B.weight({b"ab": n}) == B.WEIGHT_LIMIT - 2
    c = bpe_amd.WordCounter().add_counts({b"ab": n})
    assert c.counts() == {b"ab": n} and c.info()["n_pretokens"] == n
    vocab, merges = c.train(257, [])
    assert merges == [(b"a", b"b")] and vocab[256] == b"ab" and len(vocab) == 257
    assert _logged_counts(log) == [n]
    assert last_train_stats()["n_pretokens"] == n


REFUSED = [{b"ab": 1 << 61},                    # weight exactly 2^62
           {b"ab": (1 << 64) - 1},              # count * length overflows 64 bits
           {b"abc": -(-(1 << 64) // 3)},        # ceil(2^64 / 3): the product wraps to a small number
           {b"ab": 1 << 60, b"cd": 1 << 60},    # only the blob's sum reaches it
           {b"ab": 1 << 63, b"cd": 1 << 63}]    # the blob's sum overflows 64 bits


@pytest.mark.parametrize("counts", REFUSED, ids=["2^62", "2^64-1", "ceil(2^64/3)", "sum", "sum-wraps"])
@pytest.mark.parametrize("held", [{}, {b" held": 5, b"ab": 3}], ids=["empty", "holding"])
def test_refused_at_the_limit(counts, held):
    assert B.weight(counts) >= B.WEIGHT_LIMIT
    c = bpe_amd.WordCounter().add_counts(held)
    before, info = c.counts(), c.info()
    with pytest.raises(RuntimeError, match=LIMIT_ERROR):
        c.add_counts(counts)
    assert c.counts() == before == held and c.info() == info
    if held:
        assert c.train(258, []) == B.train_counts(held, 258)


def test_refused_when_only_the_sum_passes_the_limit():
    half = {b"ab": 1 << 60}                      # weight 2^61
    first = {b"ab": (1 << 60) - 1, b"xyz": 1}    # weight 2^61 + 1
    assert B.weight(half) + B.weight(first) == B.WEIGHT_LIMIT + 1
    c = bpe_amd.WordCounter().add_counts(first)
    info = c.info()
    with pytest.raises(RuntimeError, match=LIMIT_ERROR):
        c.add_counts(half)
    other = bpe_amd.WordCounter().add_counts(half)
    with pytest.raises(RuntimeError, match=LIMIT_ERROR):
        c.absorb(other)
    assert c.counts() == first and c.info() == info
    assert other.counts() == half
    c.add_counts({b"ab": (1 << 60) - 2})
    assert B.weight(c.counts()) == B.WEIGHT_LIMIT - 3
    with pytest.raises(RuntimeError, match=LIMIT_ERROR):
        c.add_counts({b"xyz": 1})                # 3 more: 2^62 exactly
    c.add_counts({b"ab": 1})                     # 2 more: 2^62 - 1
    assert c.counts() == {b"ab": (1 << 61) - 2, b"xyz": 1}
    assert c.train(258, [])[1] == [(b"a", b"b"), (b"y", b"z")]
