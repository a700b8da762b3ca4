"""GPU: the word counter (csrc/count.hip, table_add of csrc/stage.h) at the capacity edges of its
record aggregation, on the inputs of tests/count_cases.py; tests/test_count_cases.py shows on the
CPU which threshold each of them reaches.  Every expectation is there twice: the oracle's word
table and the case's planned multiset, which owes nothing to the oracle.

  word tables    bpe_word_counts of every case against both, as whole dicts, with no record pool,
                 with BPE355_REC_POOL=1e8, with that and the knobs the case is meant for
                 (BPE355_STREAM_WG, BPE355_LONG_SEG), and with a pool of 150 000 records that is
                 spent part way
  training       oracle.train_raw at vocab 600 through train_bpe_bytes and through train_bpe(path)
                 with BPE355_SEG_MB=1 and BPE355_AGG_SEGS=1 for one_fine_bin, the largest
                 one_coarse_bin, dense_two_byte and long_distinct (pool on, the case's knobs), and
                 through train_bpe_device on a pointer 3 bytes past a 16-byte boundary
  witnesses      last_train_stats()["n_count_records"] with the pool on: equal to the number of
                 words for one_coarse_bin (every occurrence is one record), at least the distinct
                 words for one_fine_bin, at least half the six words' occurrences for cache_set
  overflow       BPE355_WORD_CAP_LOG2=10 on the largest one_coarse_bin text (the table is counted
                 again five times): the bytes path with records on, the file path with and without
                 records, WordCounter.add_file in 256 KiB windows, then counts() and train()

No test failed on the library as it stood.  Held once against four deliberately wrong builds of
csrc/count.hip (scratch copies), to see that the cases bite; each lost counts in the tests named:
  k_rec_reduce without its table_add fallback      38 of 86: one_fine_bin with every pool, and every
                 case in which many threads meet one word at once (hot_word, dense_two_byte,
                 cache_set, packed_twins, long_distinct): a slot being claimed is passed over, so
                 the probe limit is also reached long before the LDS table is full
  spill taking c <= (1 << kCntBits) for a record   2: hot_word_3_at and hot_word_11_at with the pool
                 and one workgroup, the only runs in which one entry is flushed with exactly 2^19
  k_rec_tiles' last tile one record short          67: every test that runs with a pool
  k_count_long without its table_add fallback      8: long_distinct and packed_twins with a pool

Measured on an MI355X: the 86 tests take 6.7 s together; the slowest is
test_overflow_bytes_with_records (1.8 s: the table is counted six times, twice over), then the
first test (1.3 s of set-up loading the library, 0.7 s building the candidate table); every other
takes 0.13 s or less, reference runs included.
"""
from __future__ import annotations

import functools

import pytest

import count_cases as C
from oracle import oracle

pytestmark = pytest.mark.gpu

bpe_amd = pytest.importorskip("bpe_amd")
from bpe_amd import _lib  # noqa: E402
from bpe_amd.train import last_train_stats  # noqa: E402
from test_gpu_utf8 import _device_word_counts  # noqa: E402

POOLS = ["none", "pool", "pool_knobs", "pool_spent"]


@pytest.fixture(scope="module", autouse=True)
def _device():
    _lib.require_device()


@pytest.fixture
def knob(monkeypatch):
    def set_(k, v):
        monkeypatch.setenv(k, str(v))
    return set_


def _configure(knob, case, how):
    if how in ("pool", "pool_knobs"):
        knob("BPE355_REC_POOL", "1e8")
    if how == "pool_spent":
        knob("BPE355_REC_POOL", "150000")
    if how == "pool_knobs":
        for k, v in case.knobs.items():
            knob(k, v)


@functools.lru_cache(maxsize=None)
def _want_words(name):
    """the pre-tokens of two bytes and more: the oracle's table, equal to the plan"""
    c = C.CASES[name]()
    want = {w: n for w, n in oracle.word_counts(c.data).items() if len(w) > 1}
    assert want == c.words()
    return want


@functools.lru_cache(maxsize=None)
def _want_train(name):
    return oracle.train_raw(C.CASES[name]().data, C.TRAIN_VOCAB, [])


def _same_words(got, want):
    if got != want:
        lost = {w: (got.get(w), n) for w, n in want.items() if got.get(w) != n}
        extra = {w: n for w, n in got.items() if w not in want}
        some = list(lost.items())[:5]
        pytest.fail(f"{len(lost)} of {len(want)} words differ (word: got, want) {some}; {len(extra)} words too many "
                    f"{list(extra.items())[:5]}; occurrences {sum(got.values())} against {sum(want.values())}")


# ---------------------------------------------------------------------- word tables
@pytest.mark.parametrize("how", POOLS)
@pytest.mark.parametrize("name", list(C.CASES))
def test_word_table(knob, name, how):
    c = C.CASES[name]()
    _configure(knob, c, how)
    _same_words(_device_word_counts(c.data, []), _want_words(name))


# ---------------------------------------------------------------------- training
def _witness(name, st):
    """what the case section derives for the record count, with the pool on and not spent"""
    c = C.CASES[name]()
    records = st["n_count_records"]
    if c.family == "one_coarse_bin":
        assert records == sum(c.words().values()) == c.claims["records"] + 2
    elif c.family == "one_fine_bin":
        assert records >= len(c.words()) > c.claims["distinct"] > C.K_RED_SLOTS
    elif c.family == "cache_set":
        assert records >= sum(c.plan[w] for w in c.claims["six"]) // 2
    else:
        assert records > 0


@pytest.mark.parametrize("name", C.TRAIN_CASES + ["cache_set", "one_coarse_bin_tile", "one_coarse_bin_tile_plus_1"])
def test_train_bytes(knob, name):
    c = C.CASES[name]()
    _configure(knob, c, "pool_knobs")
    got = bpe_amd.train_bpe_bytes(c.data, C.TRAIN_VOCAB, [])
    _witness(name, last_train_stats())
    assert got == _want_train(name)


def test_records_with_the_default_grid(knob):
    """the same witnesses with every workgroup of the default grid holding a page"""
    knob("BPE355_REC_POOL", "1e8")
    for name in (C.LARGEST_COARSE, "cache_set", "one_fine_bin"):
        assert bpe_amd.train_bpe_bytes(C.CASES[name]().data, C.TRAIN_VOCAB, []) == _want_train(name)
        _witness(name, last_train_stats())


@pytest.mark.parametrize("name", C.TRAIN_CASES)
def test_train_file_segments(knob, tmp_path, name):
    c = C.CASES[name]()
    _configure(knob, c, "pool_knobs")
    knob("BPE355_SEG_MB", 1)
    knob("BPE355_AGG_SEGS", 1)
    p = tmp_path / "text.txt"
    p.write_bytes(c.data)
    got = bpe_amd.train_bpe(p, C.TRAIN_VOCAB, [])
    st = last_train_stats()
    _witness(name, st)
    if len(c.data) > (3 << 19):      # more than one segment: a partial aggregation between them
        assert st["n_count_batches"] >= 2
    assert got == _want_train(name)


def test_train_device_unaligned(knob):
    import torch
    name = "dense_two_byte_wg4"
    c = C.CASES[name]()
    _configure(knob, c, "pool_knobs")
    shift = 3
    buf = torch.zeros(len(c.data) + 16, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[shift:shift + len(c.data)] = torch.frombuffer(bytearray(c.data), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    got = bpe_amd.train_bpe_device(buf.data_ptr() + shift, len(c.data), C.TRAIN_VOCAB, [])
    assert last_train_stats()["n_count_records"] > 0
    assert got == _want_train(name)


# ---------------------------------------------------------------------- word-table overflow
def test_overflow_bytes_with_records(knob):
    name = C.LARGEST_COARSE
    c = C.CASES[name]()
    knob("BPE355_WORD_CAP_LOG2", 10)
    knob("BPE355_REC_POOL", "1e8")
    _same_words(_device_word_counts(c.data, []), _want_words(name))
    assert bpe_amd.train_bpe_bytes(c.data, C.TRAIN_VOCAB, []) == _want_train(name)
    st = last_train_stats()
    assert st["n_words"] == len(c.words())
    _witness(name, st)               # the records of the last count, the one that fitted


@pytest.mark.parametrize("records", [False, True])
def test_overflow_file_path(knob, tmp_path, records):
    """the segments' count overflows; the resident text is then counted whole"""
    name = C.LARGEST_COARSE
    c = C.CASES[name]()
    knob("BPE355_WORD_CAP_LOG2", 10)
    knob("BPE355_SEG_MB", 1)
    if records:
        knob("BPE355_REC_POOL", "1e8")
    p = tmp_path / "text.txt"
    p.write_bytes(c.data)
    assert bpe_amd.train_bpe(p, C.TRAIN_VOCAB, []) == _want_train(name)
    st = last_train_stats()
    assert st["n_words"] == len(c.words())
    if records:
        _witness(name, st)
    else:
        assert st["n_count_records"] == 0


@pytest.mark.parametrize("records", [False, True])
def test_overflow_counter_windows(knob, tmp_path, records):
    name = C.LARGEST_COARSE
    c = C.CASES[name]()
    knob("BPE355_WORD_CAP_LOG2", 10)
    if records:
        knob("BPE355_REC_POOL", "1e8")
    p = tmp_path / "text.txt"
    p.write_bytes(c.data)
    with bpe_amd.WordCounter() as counter:
        counter.add_file(p, 256 << 10)
        info = counter.info()
        assert info["n_windows"] >= 4 and info["n_words"] == len(c.words())
        _same_words(counter.counts(), _want_words(name))
        assert counter.train(C.TRAIN_VOCAB, []) == _want_train(name)
