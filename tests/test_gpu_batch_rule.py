"""GPU: the batched merge trip on word counts built to reach every way a batch forms and ends
(tests/batch_rule_cases.py; tests/test_batch_rule_cases.py shows on the CPU that the cases are what
they claim and that the rule restated there agrees with the reference trainer).  Every run writes
the round log and the trip log (8 int32 per trip: round, k, full scan, list entries, tokens, |C|,
listed keys, fresh tokens; a halted trip has round -1 and k 0) and is held against
big_count_cases.train_counts:

  1  merges and vocab equal the reference's
  2  every device round's winning count equals the reference's, and the device makes exactly the
     rounds of count >= 1 (the zero-count tail is the host's)
  3  the trips with k > 0 partition those rounds contiguously
  4  rule_allows(the state at the trip's round, k) for every trip: a batch the rule forbids fails
     here even where the merges happen to agree
  5  the case's property is reached on the device, by a trip's members or boundary; and with fewer
     than 256 live keys, all listed, trip 0 is the rule's own batch
  6  each run's (round, k, boundary) list is printed

Every case runs at its own vocab and at 66 000 (the uint32_t instantiation, to exhaustion: the
zero-count tail is compared), on the default trips, the fused trip, the 64-bit global cells, the
touched-block marks from 128 tokens on with their check, and the per-round kernels (BPE355_BATCH=0:
no trip log, checks 1 and 2); pair_filter also under BPE355_BATCH=3 (below kPairFilterK: the
compare path) and cap under BPE355_BATCH=5.

Measured on an MI355X (default knobs, own vocab; (round, k, boundary) of the first trips):

  adjacent         (0,2,clash) (2,1,clash) (3,2,tie_harmless) (5,1,ran_out); 9 more merges at count 0
  adjacent3        (0,3,clash) (3,1,clash) (4,1,strict_gap) (5,1,clash) (6,2,tie_harmless) (8,1,ran_out)
  shared_a / _b    (0,4,clash) (4,3,tie_harmless) (7,2,tie_harmless) (9,1,ran_out)
  same_list        (0,4,clash) with 8 list entries, then 3, 2, 16, 16, 3 (rounds_end; 9 to exhaustion)
  multi_hit        (0,3,clash) on lists; 114 trips for 164 rounds, 789 for the 1081 device rounds to
                   exhaustion; 2 list trips and 13 (15) scans of k > 1 hold a word hit twice
  pair_filter      (0,4,clash) (4,1,clash) (5,1,clash) then 2, 2, 2, 2, 1; BPE355_BATCH=3: (0,3,cap) (3,2,clash)
  tie_kept         (0,2,tie_harmless) (2,1,p1_a_eq_b)
  tie_cut_between  (0,3,tie_seed_cut) (3,3,ran_out)
  tie_cut_at_gap   (0,2,strict_gap) (2,4,ran_out)
  cap              (0,16,cap) (16,16,cap) (32,5,rounds_end), to exhaustion (32,8,ran_out);
                   BPE355_BATCH=5: seven trips of 5, then (35,2,rounds_end)
  overflow         256 trips of k = 1 with 512 down to 257 listed keys, then 16 trips of 16

Every trip 0 with fewer than 256 live keys took the rule's own batch.  The 125 tests take 5.1 s
together, references included: the first waits 1.6 s for the device, multi_hit to exhaustion takes
0.55 s once (its reference, 2423 merges in plain Python), every other test 0.2 s or less.

That the checks bite was tried once with five libraries built wrong on purpose (none of them kept):
4' ignored in select_core fails check 4 on adjacent3, tie_cut_between and tie_cut_at_gap, where the merges
still agree, and check 1 on multi_hit; a shared slot of the pair table given to one member fails
pair_filter; dup_list ignored fails same_list alone; a token group's first member reading only its
own cells fails shared_a, shared_b, same_list and multi_hit; the apply without its |S|^2 items
fails adjacent, adjacent3 and every case with a key between two of the batch's tokens.
"""
from __future__ import annotations

import struct

import pytest

import batch_rule_cases as R

pytestmark = pytest.mark.gpu

bpe_amd = pytest.importorskip("bpe_amd")

KNOBS = [None, "BPE355_FOLD=1", "BPE355_LDS_CELLS=0",
         "BPE355_DENSE_TOK=128+BPE355_SPARSE_FROM=128+BPE355_CHECK_MARKS=1", "BPE355_BATCH=0"]
RUNS = [(case, knob) for case in R.CASES for knob in KNOBS] + \
       [(case, f"BPE355_BATCH={n}") for case, ns in R.EXTRA_BATCH.items() for n in ns]


@pytest.fixture(scope="module", autouse=True)
def _device():
    from bpe_amd import _lib
    _lib.require_device()


def _set(knob, monkeypatch):
    for kv in (knob or "").split("+"):
        if kv:
            monkeypatch.setenv(*kv.split("="))


def _cap(knob):
    return int(knob.split("=")[1]) if knob and knob.startswith("BPE355_BATCH=") else R.CAP


def _run(case, vocab, knob, tmp_path, monkeypatch):
    """(the reference's trace, the device's logged counts, its trips with k > 0) after checks 1-3."""
    _set(knob, monkeypatch)
    rlog, tlog = tmp_path / "rounds.bin", tmp_path / "trips.bin"
    monkeypatch.setenv("BPE355_ROUND_LOG", str(rlog))
    monkeypatch.setenv("BPE355_TRIP_LOG", str(tlog))
    tr = R.trace(case, vocab)
    g_vocab, g_merges = bpe_amd.train_bpe_word_counts(tr.counts, tr.vocab_size, [])
    if g_merges != tr.merges:                                            # 1
        i = next((k for k, (a, b) in enumerate(zip(g_merges, tr.merges)) if a != b),
                 min(len(g_merges), len(tr.merges)))
        pytest.fail(f"merges differ at round {i} of {len(g_merges)} / {len(tr.merges)}: device "
                    f"{g_merges[i:i + 2]!r}, reference {tr.merges[i:i + 2]!r}")
    assert g_vocab == tr.vocab
    raw = rlog.read_bytes()                                              # 2
    assert len(raw) % 24 == 0
    counts = [struct.unpack_from("<IIIIq", raw, o)[4] for o in range(0, len(raw), 24)]
    assert len(counts) == tr.n_live
    bad = [(r, g, w) for r, (g, w) in enumerate(zip(counts, tr.tops)) if g != w]
    assert not bad, f"{len(bad)} rounds with another count; the first (round, device, reference): {bad[:3]}"
    if _cap(knob) == 0:
        assert not tlog.exists()
        return tr, counts, None
    raw = tlog.read_bytes()
    assert len(raw) % 32 == 0
    recs = [struct.unpack_from("<8i", raw, o) for o in range(0, len(raw), 32)]
    assert all(t[0] == -1 for t in recs if t[1] == 0)
    trips = [t for t in recs if t[1] > 0]
    at = 0                                                               # 3
    for t in trips:
        assert t[0] == at, f"trip at round {t[0]} after the rounds up to {at}: {trips[:20]}"
        at += t[1]
    assert at == tr.n_live
    return tr, counts, trips


def _property(case, tr, trips, cap, own_vocab):
    """Check 5: what the case is for, on the device's own trips."""
    members = lambda t: tr.members(t[0], t[1])                 # noqa: E731
    bnd = lambda t: tr.boundary(t[0], t[1], cap)               # noqa: E731
    multi = [t for t in trips if t[1] > 1]
    if case in ("adjacent", "adjacent3"):
        n = 2 if case == "adjacent" else 3
        assert any(t[1] == n and R.adjacent_members(tr.words_at(t[0]), members(t)) == {"up", "down"}
                   for t in multi)
    elif case == "shared_a":
        assert any(t[1] >= 4 and R.shares_a(members(t)) for t in multi)
    elif case == "shared_b":
        assert any(t[1] >= 4 and R.shares_b(members(t)) for t in multi)
    elif case == "same_list":
        t = trips[0]
        words = tr.words_at(0)
        shared = R.same_list(words, members(t))
        z = R.posting_lengths(words)
        assert t[1] == 4 and shared == {b"t"} and t[2] == 0
        assert t[3] == z[b"t"] == 8, f"list entries {t[3]}: one walk of t's list is {z[b't']}"
    elif case == "multi_hit":
        hit2 = {}
        for t in multi:                                        # (rounds ascending: one replay)
            hit2[t] = sum(R.word_hit_by(tr.words_at(t[0]), members(t), 2).values())
        lists = [t for t in multi if t[2] == 0 and hit2[t]]
        scans = [t for t in multi if t[2] == 1 and hit2[t]]
        print(f"multi_hit: {len(lists)} list trips and {len(scans)} scans of k > 1 with a word hit twice")
        assert lists and scans
        assert any(t[1] >= R.PAIR_FILTER_K and t[2] == 1 and hit2[t] for t in multi)   # the pair table in a scan
        t = trips[0]
        assert t[1] == 3 and t[2] == 0 and members(t) == list(R.MULTI_MEMBERS)
        assert set(R.word_hit_by(tr.words_at(0), members(t), 3)) == {0, 1, 2, 3, 4}
    elif case == "pair_filter":
        if cap >= R.PAIR_FILTER_K:
            assert any(R.filter_collision(tr.ids, members(t)) and
                       R.filter_false_positive(tr.ids, tr.words_at(t[0]), members(t)) for t in multi)
        else:
            t = trips[0]
            assert t[1] == cap == 3 and bnd(t) == "cap"
            assert {(b"a", b"b"), (b"y", b"l")} <= set(members(t))
    elif case == "tie_kept":
        assert (trips[0][1], bnd(trips[0])) == (2, "tie_harmless")
    elif case == "tie_cut_between":
        assert (trips[0][1], bnd(trips[0])) == (3, "tie_seed_cut")
    elif case == "tie_cut_at_gap":
        assert (trips[0][1], bnd(trips[0])) == (2, "strict_gap")
    elif case == "cap":
        assert max(t[1] for t in trips) == cap and bnd(trips[0]) == "cap"
        if own_vocab:
            t = trips[-1]
            assert t[1] < min(tr.n_keys[t[0]], cap) and t[1] == tr.n_rounds - t[0] and bnd(t) == "rounds_end"
    elif case == "overflow":
        over = [t for t in trips if t[6] > R.LIST_CAP]
        after = [t for t in trips if t[0] > over[-1][0]] if over else []
        print(f"overflow: {len(over)} trips with more than {R.LIST_CAP} listed keys, then "
              f"{[t[1] for t in after]}")
        assert over and all(t[1] == 1 for t in over) and over == trips[:len(over)]
        assert all(tr.n_keys[t[0]] > R.LIST_CAP for t in over)
        assert sum(t[1] == R.CAP for t in after) >= 10
        assert all(bnd(t) == "tie_harmless" for t in after if t[1] == R.CAP and t[0] + t[1] < tr.n_live)
    else:
        raise AssertionError(case)


@pytest.mark.parametrize("vocab", ["own", R.EXHAUST_VOCAB])
@pytest.mark.parametrize("case,knob", RUNS)
def test_batch_rule(case, knob, vocab, tmp_path, monkeypatch):
    own = vocab == "own"
    cap = _cap(knob)
    tr, _counts, trips = _run(case, None if own else vocab, knob, tmp_path, monkeypatch)
    if not own:   # the pairs ran out; the adjacent cases' transient keys are popped at count 0
        assert tr.n_live <= len(tr.merges) < vocab - 256
        assert tr.n_live + 9 <= len(tr.merges) or not case.startswith("adjacent")
    if trips is None:
        return
    ends = [(t[0], t[1], "list_overflow" if t[6] > R.LIST_CAP else tr.boundary(t[0], t[1], cap)) for t in trips]
    print(f"{case} {knob} {vocab}:", ends[:40], f"({len(trips)} trips)")                      # 6
    assert max(t[1] for t in trips) <= cap
    bad = [t for t in trips if not tr.allows(t[0], t[1])]                                    # 4
    assert not bad, f"trips the batch rule forbids (round, k, ...): {bad[:5]}"
    if tr.n_keys[0] < R.LIST_CAP:   # every key is listed: the first trip is the rule's own batch
        g = min(R.greedy_k(tr.views[0], tr.present(0), cap)[0], tr.n_rounds)
        assert trips[0][1] == g and trips[0][6] == tr.n_keys[0], (trips[0], g, tr.n_keys[0])
    _property(case, tr, trips, cap, own)                                                     # 5


def test_trips_differ_from_single_merges(tmp_path, monkeypatch):
    """The checks above are not vacuous: with one member per trip (BPE355_BATCH=1) the same case has
    as many trips as rounds, so check 5 would fail; and the trip log's fields are what they are
    read as (tokens = 256 + round, fresh = k)."""
    tr, _counts, trips = _run("cap", None, "BPE355_BATCH=1", tmp_path, monkeypatch)
    assert [t[:2] for t in trips] == [(r, 1) for r in range(tr.n_live)]
    assert all(t[4] == 256 + t[0] and t[7] == 1 for t in trips)
    with pytest.raises(AssertionError):
        _property("cap", tr, trips, R.CAP, True)
