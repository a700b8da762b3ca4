"""CPU: the directed cases of tests/batch_rule_cases.py are what they claim, and the batch rule
restated there is consistent with the reference trainer itself, so that test_gpu_batch_rule.py may
hold the device's trips against it.  Each test prints what it counted.
"""
from __future__ import annotations

import collections

import pytest

import batch_rule_cases as R
import big_count_cases as B
import tie_cases


def _trips(case, cap=R.CAP):
    tr = R.trace(case)
    trips = tr.greedy_trips(cap)
    print(case, "greedy trips:", trips[:12], dict(collections.Counter(b for _r, _k, b in trips)))
    assert sum(k for _r, k, _b in trips) == tr.n_live and all(b in R.BOUNDARIES for _r, _k, b in trips)
    return tr, trips


# ---------------------------------------------------------------- the rule against the reference
def _consistent(tr):
    """For every state r and every k the rule allows there, the reference's merges r .. r + k - 1
    are the top k of state r with the counts they had at r."""
    allowed = collections.Counter()
    present = tr.present(0)
    for r in range(tr.n_live):
        present.add(b"".join(tr.merges[r - 1])) if r else None
        g, k_rule, _why = R.greedy_k(tr.views[r], present)
        assert R.rule_allows(tr.views[r], present, g) and 1 <= g <= k_rule
        for k in range(1, R.CAP + 1):
            if r + k > len(tr.merges) or not R.rule_allows(tr.views[r], present, k):
                continue
            allowed[k] += 1
            top = R.ranked(tr.views[r], k)
            assert [p for _c, p in top] == tr.merges[r:r + k], (r, k)
            assert [c for c, _p in top] == tr.tops[r:r + k], (r, k)
    return allowed


@pytest.mark.parametrize("case", list(R.CASES))
def test_rule_is_consistent_with_the_reference(case):
    tr = R.trace(case)
    allowed = _consistent(tr)
    print(case, tr.n_live, "states; (state, k) allowed, by k:", sorted(allowed.items()))
    assert allowed[1] == tr.n_live


@pytest.mark.parametrize("kind", tie_cases.KINDS)
def test_rule_is_consistent_on_deep_ties(kind):
    tr = R.tie_trace(kind)
    allowed = _consistent(tr)
    trips = tr.greedy_trips()
    print(kind, tr.n_live, "states; allowed by k:", sorted(allowed.items()),
          dict(collections.Counter(b for _r, _k, b in trips)))
    assert allowed[1] == tr.n_live == tie_cases.SCALED_VOCAB - 256
    assert sum(n for k, n in allowed.items() if k > 1) > 100
    ends = {b for _r, _k, b in trips}
    assert {"clash", "strict_gap", "tie_seed_cut", "tie_harmless"} <= ends


def test_a_forbidden_batch_is_refused():
    """The rule is no rubber stamp: one more member than greedy_k's token boundary, a batch across
    a seeding tie, and the reference itself disagrees with a batch the rule refuses."""
    tr = R.trace("tie_cut_between")
    assert [tr.allows(0, k) for k in range(1, 7)] == [True, True, True, False, False, False]
    assert tr.boundary(0, 4) == "forbidden"
    tr = R.trace("adjacent")
    assert tr.allows(0, 2) and not tr.allows(0, 3)      # (b,c): its a is a member's b
    top3 = [p for _c, p in R.ranked(tr.views[0], 3)]
    assert top3 != tr.merges[:3]                        # the reference takes (ab,cd) third, a new key
    assert not R.rule_allows({(b"a", b"a"): 5, (b"b", b"c"): 4}, set(), 2)          # (2)
    assert not R.rule_allows({(b"a", b"bc"): 5, (b"ab", b"c"): 4}, set(), 2)        # (3) same bytes
    assert not R.rule_allows({(b"a", b"b"): 5, (b"c", b"d"): 4}, {b"cd"}, 2)        # (3) a token
    assert R.rule_allows({(b"a", b"b"): 5, (b"c", b"d"): 4}, {b"ab"}, 1)            # (k = 1)
    assert R.boundary({(b"a", b"b"): 5, (b"c", b"d"): 4}, {b"cd"}, 1) == "exists"
    assert R.boundary({(b"a", b"bc"): 5, (b"ab", b"c"): 4}, set(), 1) == "same_bytes"
    assert not R.rule_allows({(b"a", b"b"): 5}, set(), 2) and not R.rule_allows({(b"a", b"b"): 0}, set(), 1)


# ---------------------------------------------------------------- the cases
def test_pair_h12_collisions():
    h = lambda p: R.pair_h12(p[0], p[1])   # noqa: E731
    for group in ((b"ab", b"yl"), (b"ar", b"cl"), (b"be", b"pl"), (b"al", b"cr", b"yb")):
        assert len({h(p) for p in group}) == 1, group
    assert len({h(p) for p in (b"ab", b"ar", b"be", b"al", b"mn")}) == 5
    assert R.pair_h12(0xFFFFFFFF, 0xFFFFFFFF) == ((0x61C8864F ^ 0x7A143589) >> 20)   # 32-bit wrap


@pytest.mark.parametrize("case,n", [("adjacent", 2), ("adjacent3", 3)])
def test_adjacent(case, n):
    tr, trips = _trips(case)
    assert trips[0][:2] == (0, n) and trips[0][2] == "clash"
    members = tr.members(0, n)
    assert R.adjacent_members(tr.words_at(0), members) == {"up", "down"}
    # a key between two new tokens does not exist before the trip and is live after it
    new = [a + b for a, b in members]
    assert not any((x, y) in tr.views[0] for x in new for y in new)
    assert any(x in new and y in new for x, y in tr.merges[n:tr.n_live])


def test_adjacent_zero_count_tail():
    tr = R.trace("adjacent", R.EXHAUST_VOCAB)
    zero = [m for m, c in zip(tr.merges, tr.tops) if c == 0]
    print("adjacent to exhaustion:", len(tr.merges), "merges,", len(zero), "at count 0:", zero)
    assert len(tr.merges) == 15 and len(zero) == 9 and tr.tops == sorted(tr.tops, reverse=True)
    assert set(R.ADJACENT_ZERO_MERGES) <= set(zero)
    tr3 = R.trace("adjacent3", R.EXHAUST_VOCAB)
    assert sum(c == 0 for c in tr3.tops) >= 9


@pytest.mark.parametrize("case,pred,letter", [("shared_a", R.shares_a, b"t"), ("shared_b", R.shares_b, b"e")])
def test_shared_token(case, pred, letter):
    tr, trips = _trips(case)
    assert trips[0][:2] == (0, 4)
    members = tr.members(0, 4)
    assert pred(members) and {letter} == ({a for a, _ in members} if case == "shared_a" else {b for _, b in members})
    # a neighbour key of the shared token receives deltas from at least three members
    words = tr.words_at(0)
    side = (lambda w, q: w[q - 1] if q else None) if case == "shared_a" else \
           (lambda w, q: w[q + 2] if q + 2 < len(w) else None)
    got = collections.defaultdict(set)
    for w in words:
        for q in range(len(w) - 1):
            if (w[q], w[q + 1]) in members and side(w, q) is not None:
                got[side(w, q)].add((w[q], w[q + 1]))
    print(case, "neighbours -> members:", {k: len(v) for k, v in got.items()})
    assert max(len(v) for v in got.values()) >= 3


def test_same_list():
    tr, trips = _trips("same_list")
    assert trips[0][:2] == (0, 4) and tr.n_keys[0] < R.LIST_CAP
    words, members = tr.words_at(0), tr.members(0, 4)
    z = R.posting_lengths(words)
    assert R.same_list(words, members) == {b"t"}
    assert z[b"t"] == 8 <= len(words) // 4 and all(z[v] == 12 for v in (b"a", b"e", b"i", b"o"))
    assert R.walks_lists(tr, 0, 4)
    assert R.same_list(R.trace("shared_a").words_at(0), members) == set()   # there the second letters' lists


def test_multi_hit():
    tr, trips = _trips("multi_hit")
    assert trips[0] == (0, 3, "clash") and tr.members(0, 3) == list(R.MULTI_MEMBERS)
    assert tr.n_keys[0] < R.LIST_CAP and tr.n_live == tr.n_rounds < 256
    words, members = tr.words_at(0), tr.members(0, 3)
    by3 = R.word_hit_by(words, members, 3)
    print("multi_hit: words holding all three members, by class:", by3)
    assert all(by3.get(c, 0) >= 2 for c in range(5))
    multi = [w for w in words if R.hits(w, members) == 3]
    assert all((w[0], w[1]) == members[0] and (w[-2], w[-1]) == members[2] for w in multi)   # first, last pair
    assert sum(list(zip(w, w[1:])).count(members[0]) == 2 for w in multi) >= 10               # one member twice
    assert all([a, b] in words for a, b in members)                                          # 2-id words
    # both ways to find the words, each with a word that several members hit
    lists = [(r, k) for r, k, _b in trips if k > 1 and R.walks_lists(tr, r, k)]
    scans = [(r, k) for r, k, _b in trips if k > 1 and not R.walks_lists(tr, r, k)]
    hit2 = lambda r, k: sum(R.word_hit_by(tr.words_at(r), tr.members(r, k), 2).values())   # noqa: E731
    print("multi_hit: trips of k > 1 that walk lists:", lists[:5], len(lists), "that scan:", scans[:5], len(scans))
    assert (0, 3) in lists and hit2(0, 3) >= len(R.MULTI_LENGTHS)
    assert sum(hit2(r, k) > 0 for r, k in scans) >= 3
    assert sum(k >= R.PAIR_FILTER_K and hit2(r, k) > 0 for r, k in scans) >= 3   # the pair table in a scan
    # later batches hit words of the 64-id class and the long table several times too
    late = collections.Counter()
    for r, k in scans:
        late.update(R.word_hit_by(tr.words_at(r), tr.members(r, k), 2).keys())
    print("multi_hit: scanning trips with a word hit twice, by class:", dict(late))
    assert late[3] >= 1 and late[4] >= 1


def test_pair_filter():
    tr, trips = _trips("pair_filter")
    assert trips[0] == (0, 4, "clash") and tr.members(0, 4) == list(R.PAIR_FILTER_MEMBERS)
    words, members = tr.words_at(0), tr.members(0, 4)
    assert R.filter_collision(tr.ids, members)
    fp = R.filter_false_positive(tr.ids, words, members)
    print("pair_filter: non-member pairs in a member's slot:", fp)
    assert fp == {(b"a", b"l"), (b"y", b"b")}
    assert any(R.hits(w, members) >= 3 for w in words)                      # a word with the shared slot and more
    assert [b"a", b"b", b"y", b"l"] in words                                # both sharers of a slot, adjacent
    # under a cap of 3 the compare path runs: no table
    _tr, trips3 = _trips("pair_filter", 3)
    assert trips3[0] == (0, 3, "cap") and not R.filter_collision(tr.ids, members[:3])


def test_tie_boundaries():
    tr, trips = _trips("tie_kept")
    assert trips[0] == (0, 2, "tie_harmless") and R.greedy_k(tr.views[0], tr.present(0)) == (2, 2, "a_eq_b")
    tr, trips = _trips("tie_cut_between")
    assert trips[0] == (0, 3, "tie_seed_cut")
    assert R.greedy_k(tr.views[0], tr.present(0)) == (3, 5, "clash")       # strict gap at 1 < 3 < 5
    assert [c for c, _p in R.ranked(tr.views[0], 6)] == [100, 90, 90, 90, 90, 90]
    tr, trips = _trips("tie_cut_at_gap")
    assert trips[0] == (0, 2, "strict_gap")
    assert R.greedy_k(tr.views[0], tr.present(0)) == (2, 5, "clash")
    assert [c for c, _p in R.ranked(tr.views[0], 6)] == [100, 95, 90, 90, 90, 90]
    assert R._first_seeded(tr.views[0], tr.members(0, 5), 90) == 0         # the seed is above the gap


def test_cap():
    tr, trips = _trips("cap")
    assert trips == [(0, 16, "cap"), (16, 16, "cap"), (32, 5, "rounds_end")]
    assert tr.n_keys[32] == 8 and R.greedy_k(tr.views[32], tr.present(32))[0] == 8
    _tr, trips5 = _trips("cap", 5)
    assert [k for _r, k, _b in trips5] == [5] * 7 + [2] and trips5[-1][2] == "rounds_end"


def test_overflow():
    tr, trips = _trips("overflow")
    assert tr.n_keys[0] == 512 and tr.n_keys[256] == 256 == R.LIST_CAP and tr.n_keys[255] > R.LIST_CAP
    assert all(k == 16 for _r, k, _b in trips) and {b for _r, _k, b in trips} == {"tie_harmless", "cap"}
    assert tr.merges[0] == (b"\xbf", b"\xc7") and tr.merges == sorted(tr.merges, reverse=True)
    assert set(tr.tops) == {1000}


def test_every_boundary_but_rule_3_is_reached():
    seen = collections.Counter()
    for case in R.CASES:
        seen.update(b for _r, _k, b in R.trace(case).greedy_trips())
    seen.update(b for _r, _k, b in R.trace("cap").greedy_trips(5))
    print(dict(seen))
    assert set(seen) == set(R.BOUNDARIES) - {"exists", "same_bytes"}


def test_cases_are_small():
    for case, build in R.CASES.items():
        counts, vocab = build()
        assert len(counts) <= 520 and vocab - 256 <= 1300, case
        assert case == "overflow" or R.trace(case).n_keys[0] < R.LIST_CAP, case
        assert B.weight(counts) < 1 << 31


def test_no_training_run_makes_the_same_bytes_twice():
    """A slice (every eighth seed) of the 10 000 corpora of the module docstring's search."""
    found = [s for s in range(0, 10_000, 8) if R.makes_same_bytes_twice(*R.random_small_corpus(s))]
    assert not found
    assert sum(bool(R.random_small_corpus(s)[1]) for s in range(100)) == 50
