"""The batch rule of the merge loop restated, and word counts built to reach every way a batch of
up to 16 merges forms and ends (csrc/train_select.h, train_merge.h, train_apply.h).

The inputs are {bytes: int} word counts, trained with bpe_amd.train_bpe_word_counts, so pair counts
and ties are exact by construction.  The reference is big_count_cases.train_counts, whose on_round
hook hands over the `pairs` dict before every round.

The rule is restated here from the comment at the top of train_select.h ((1)-(4) and the tie rule
(4')), not from select_core:

  rule_allows(pairs, present, k)   may the top k keys of this state be merged in one trip?
  greedy_k(pairs, present, cap)    the longest batch the rule gives when every key is listed, with
                                   (4') applied at the token rules' own boundary as the code does
  boundary(pairs, present, k)      what stopped the batch at k (see BOUNDARIES)

A device trip may take fewer members than greedy_k (its candidate list ran out, its list overflowed,
the rounds ended) and, because (4') is applied only at the trip's own boundary, even more (a list
that ran out at 6 across a harmless tie, where the full list's boundary at 9 is cut back to 4 by a
seeding tie).  So the check of a device trip is rule_allows at its own k, never k <= greedy_k.

Trace(counts, vocab) runs the reference once and keeps, per round, what the rule reads of the state
(view), the words (words_at) and the token ids (ids: the byte value, then 256 + n for the n-th new
token), for the predicates on a batch:

  shares_a / shares_b      at least 3 members with one a / one b (the ga / gb group masks)
  adjacent_members         a word holds a_i b_i a_j b_j consecutively, for i < j and for i > j (the
                           key (new_i, new_j) is made and emptied within the trip)
  same_list                two members whose shorter posting list is the same token's (dup_list)
  word_hit_by(n)           words holding at least n members, per slot class
  filter_collision         two of at least kPairFilterK = 4 members with equal pair_h12 (0xFF slots)
  filter_false_positive    a rewritten word holds a non-member pair in a member's slot

The directed cases (CASES: name -> (counts, vocab)); test_batch_rule_cases.py shows on the CPU that
each is what it claims:

  adjacent, adjacent3   two / three members adjacent inside words, in both rank orders; run to
                        exhaustion the reference pops the transient keys at count 0
  shared_a, shared_b    four members with one a / one b; the neighbour keys (x, t) / (e, x) receive
                        deltas from several members
  same_list             shared_a among 40 words that hold the second letters without "t": t's list
                        is the shorter one of all four members
  multi_hit             words of 6 to 100 ids holding three members (one of them twice, hits on the
                        first and the last pair), 2-id words equal to a member, among 240 words
                        over four other letters: trip 0 walks posting lists, later trips scan
  pair_filter           four members, two of them in one slot of the rewrite's pair table, and
                        words holding a non-member pair that hashes to a member's slot
  tie_kept, tie_cut_between, tie_cut_at_gap
                        a tie at the boundary that is kept; one cut at the member a tied key seeds,
                        between the strict gap and the token rules' k; one whose seeded member lies
                        above the strict gap, so the batch ends at the gap
  cap                   40 disjoint pairs of distinct counts, 37 rounds: trips of 16, 16 and 5, the
                        last cut by the rounds left with 8 candidates listed
  overflow              512 disjoint pairs of one count: more than kListCap = 256 keys are listed
                        until 256 are popped (P1 alone, ordered by high bytes), then 16 at a time
                        across harmless ties

Not reachable, so not a case: rule (3).  A search of 10 000 random corpora (1 to 6 words of 2 to 12
letters over "a", "ab", "abc", "aab" and "abcd", counts 1 to 5, half of them with a special token
cut from one of the words) trained until no pair is left, zero-count merges included, found no run
in which a + b is an existing token or two merges make the same bytes
(test_batch_rule_cases.py::test_no_training_run_makes_the_same_bytes_twice repeats a slice of it).
The special tokens are put into the vocab on the host after the loop, so the device's dedupe path
(cand_meta's map_find, the byte compare in the clash check) is not reached from any input.
"""
from __future__ import annotations

import functools
import heapq
import random

import big_count_cases as B
from synth_text import SplitMix64

CAP = 16                 # kMaxBatch
LIST_CAP = 256           # kListCap
PAIR_FILTER_K = 4        # kPairFilterK
BOUNDARIES = ("cap", "ran_out", "a_eq_b", "clash", "exists", "same_bytes", "strict_gap",
              "tie_seed_cut", "tie_harmless", "p1_a_eq_b", "rounds_end")
EXHAUST_VOCAB = 66_000   # uint32_t ids, and every case runs out of pairs long before


# ---------------------------------------------------------------- the rule
def ranked(pairs, n):
    """The first n keys of count >= 1 in the reference's order: [(count, (a, b))], greatest first."""
    return heapq.nlargest(n, ((c, p) for p, c in pairs.items() if c >= 1))


def _token_stop(top, present, cap):
    """(k, why): the longest prefix of `top` that rules (1)-(3) and the cap admit, and what ended it."""
    if not top:
        return 0, "ran_out"
    a1, b1 = top[0][1]
    if a1 == b1:
        return 1, "p1_a_eq_b"
    if a1 + b1 in present:
        return 1, "exists"
    As, Bs, new = {a1}, {b1}, {a1 + b1}
    k = 1
    while True:
        if k == cap:
            return k, "cap"
        if k == len(top):
            return k, "ran_out"
        a, b = top[k][1]
        if a == b:
            return k, "a_eq_b"
        if a + b in present:
            return k, "exists"
        if a + b in new:
            return k, "same_bytes"
        if a in Bs or b in As:
            return k, "clash"
        As.add(a); Bs.add(b); new.add(a + b)
        k += 1


def _first_seeded(pairs, members, c):
    """The first member (rank from 0) whose new pairs a non-member key of count c could seed: the
    key ends in that member's a or begins with its b.  len(members): none."""
    mset = set(members)
    jb = len(members)
    for y, cy in pairs.items():
        if cy != c or y in mset:
            continue
        for j, (a, b) in enumerate(members[:jb]):
            if y[1] == a or y[0] == b:
                jb = j
                break
    return jb


def rule_allows(pairs, present, k) -> bool:
    """May the top k keys (count >= 1) of the state `pairs` (with the tokens `present`) form one
    batch?  (1) no member's b is any member's a, (2) a != b, (3) the new byte strings differ from
    each other and from every token -- all three only for k > 1 --, (4) the k-th count is strictly
    above the next key's, or (4') at a tie no tied non-member ends in a_j or begins with b_j for a
    member j, unless j is the last member (the first such j: k <= j + 1)."""
    if not 1 <= k <= CAP:
        return False
    top = ranked(pairs, k + 1)
    if len(top) < k:
        return False
    members = [p for _c, p in top[:k]]
    if k > 1:
        if any(a == b for a, b in members):
            return False
        if {a for a, _b in members} & {b for _a, b in members}:
            return False
        new = [a + b for a, b in members]
        if len(set(new)) < k or any(t in present for t in new):
            return False
    c = top[k - 1][0]
    if len(top) == k or c > top[k][0]:
        return True
    return k <= _first_seeded(pairs, members, c) + 1


def greedy_k(pairs, present, cap=CAP):
    """(k, k_rule, why): the batch of the rule with every key listed.  k_rule is where rules
    (1)-(3) or the cap end the batch and `why` what ended it there; k is k_rule cut back to the
    strict gap below it, or, with a tie at k_rule, to the first member a tied key seeds."""
    top = ranked(pairs, cap + 1)
    k, why = _token_stop(top, present, cap)
    if k <= 1:
        return k, k, why
    cnt = lambda i: top[i][0] if i < len(top) else 0   # noqa: E731
    ks = k
    while ks > 1 and not cnt(ks - 1) > cnt(ks):
        ks -= 1
    if ks == k:
        return k, k, why
    jb = _first_seeded(pairs, [p for _c, p in top[:k]], cnt(k - 1))
    return min(k, max(jb + 1, ks)), k, why


def boundary(pairs, present, k, cap=CAP, rounds_left=None) -> str:
    """What stopped the batch at k (one of BOUNDARIES), or "forbidden" if the rule does not allow k.
    With k where rules (1)-(3) or the cap end the batch: "tie_harmless" if the k-th count ties with
    the next key's (the tie was kept), else that rule.  Below it: "rounds_end" when k is the rounds
    left, "strict_gap" when the k-th count is strictly above the next, else "tie_seed_cut"."""
    if not rule_allows(pairs, present, k):
        return "forbidden"
    top = ranked(pairs, cap + 1)
    k_rule, why = _token_stop(top, present, cap)
    tie = k < len(top) and top[k - 1][0] == top[k][0]
    if k >= k_rule:
        return "tie_harmless" if tie and k > 1 else why
    if rounds_left is not None and k == rounds_left:
        return "rounds_end"
    return "tie_seed_cut" if tie else "strict_gap"


def view(pairs) -> dict:
    """The part of a state that the rule reads: the first CAP + 1 keys and every key tied with one."""
    cs = {c for c, _p in ranked(pairs, CAP + 1)}
    return {p: c for p, c in pairs.items() if c in cs}


# ---------------------------------------------------------------- a reference run, kept
def pair_h12(x: int, y: int) -> int:
    """The slot of the pair (x, y) of token ids in the rewrite's pair table (train_select.h)."""
    return ((((x * 0x9E3779B1) & 0xFFFFFFFF) ^ ((y * 0x85EBCA77) & 0xFFFFFFFF)) >> 20) & 0xFFF


def _merge_word(w, a, b, new):
    out, i, n = [], 0, len(w)
    while i < n:
        if i + 1 < n and w[i] == a and w[i + 1] == b:
            out.append(new)
            i += 2
        else:
            out.append(w[i])
            i += 1
    return out


class Trace:
    """One run of the reference on `counts`: merges, vocab, each round's winning count (tops), what
    the rule reads of each round's state (views), and the words at any round."""

    def __init__(self, counts, vocab_size):
        self.counts, self.vocab_size = counts, vocab_size
        self.views, self.tops, self.n_keys = [], [], []

        def on_round(pairs, best):
            self.views.append(view(pairs))
            self.tops.append(pairs[best])
            self.n_keys.append(sum(c >= 1 for c in pairs.values()))
        self.vocab, self.merges = B.train_counts(counts, vocab_size, (), on_round)
        self.ids = {tok: i for i, tok in self.vocab.items()}
        self.n_live = sum(c >= 1 for c in self.tops)     # the rounds a device makes itself
        self.n_rounds = vocab_size - 256                 # the rounds asked for
        self._words = [[bytes([x]) for x in w] for w, c in counts.items() if c and len(w) >= 2]
        self.freq = [c for w, c in counts.items() if c and len(w) >= 2]
        self._at = 0

    def present(self, r):
        return {bytes([i]) for i in range(256)} | {a + b for a, b in self.merges[:r]}

    def members(self, r, k):
        return [p for _c, p in ranked(self.views[r], k)]

    def words_at(self, r):
        """The words (lists of tokens, in the order of self.freq) before round r."""
        if r < self._at:
            self._words = [[bytes([x]) for x in w] for w, c in self.counts.items() if c and len(w) >= 2]
            self._at = 0
        while self._at < r:
            a, b = self.merges[self._at]
            self._words = [_merge_word(w, a, b, a + b) if a in w else w for w in self._words]
            self._at += 1
        return self._words

    def allows(self, r, k):
        return rule_allows(self.views[r], self.present(r), k)

    def boundary(self, r, k, cap=CAP):
        return boundary(self.views[r], self.present(r), k, cap, self.n_rounds - r)

    def greedy_trips(self, cap=CAP):
        """[(round, k, boundary)] of the rule with every key listed, over the rounds of count >= 1."""
        out, r = [], 0
        while r < self.n_live:
            k = min(greedy_k(self.views[r], self.present(r), cap)[0], self.n_rounds - r)
            out.append((r, k, self.boundary(r, k, cap)))
            r += k
        return out


# ---------------------------------------------------------------- predicates on a batch
def shares_a(members) -> bool:
    return any(sum(a == x for a, _b in members) >= 3 for x, _y in members)


def shares_b(members) -> bool:
    return any(sum(b == y for _a, b in members) >= 3 for _x, y in members)


def adjacent_members(words, members):
    """{"up", "down"}: a word holds a_i b_i a_j b_j consecutively with i < j ("up"), with i > j."""
    rank = {p: j for j, p in enumerate(members)}
    out = set()
    for w in words:
        for q in range(len(w) - 3):
            i, j = rank.get((w[q], w[q + 1])), rank.get((w[q + 2], w[q + 3]))
            if i is not None and j is not None and i != j:
                out.add("up" if i < j else "down")
    return out


def hits(word, members) -> int:
    """How many of the members the word holds."""
    have = set(zip(word, word[1:]))
    return sum(p in have for p in members)


def word_hit_by(words, members, n) -> dict:
    """{slot class (4: the long table): words holding at least n members}, by the words' lengths
    in this state (the device's class is that of the last compaction: the same in round 0)."""
    out = {}
    for w in words:
        if len(w) >= 2 and hits(w, members) >= n:
            out[B.class_of(len(w))] = out.get(B.class_of(len(w)), 0) + 1
    return out


def posting_lengths(words) -> dict:
    """{token: the words under 64 ids that hold it}: the posting lists of an index built now."""
    out = {}
    for w in words:
        if 2 <= len(w) < 64:
            for t in set(w):
                out[t] = out.get(t, 0) + 1
    return out


def same_list(words, members):
    """The tokens whose posting list is the shorter one (a's at equal lengths) of two or more
    members: the later member walks none of it."""
    z = posting_lengths(words)
    walked = [a if z.get(a, 0) <= z.get(b, 0) else b for a, b in members]
    return {t for t in walked if walked.count(t) >= 2}


def walks_lists(tr: "Trace", r, k) -> bool:
    """A model of the select's choice between the members' posting lists and one scan of every
    word, for a trip before the first compaction (round 256 at the earliest): the index is that of
    round 0, a token made since is covered by the shorter list of its two parts, a list longer
    than a quarter of the words under 64 ids is not walked, nor are the members' lists together
    when they pass that length (a list two members share counts once)."""
    assert r + k <= 256
    words = tr.words_at(0)
    z = posting_lengths(words)
    n = sum(2 <= len(w) < 64 for w in words)
    cover = {}

    def cov(t):   # (the token whose list covers t, its length)
        if len(t) == 1:
            return t, z.get(t, 0)
        if t not in cover:
            a, b = next(m for m in tr.merges if m[0] + m[1] == t)
            ca, cb = cov(a), cov(b)
            cover[t] = ca if ca[1] <= cb[1] else cb
        return cover[t]
    lists = {}
    for a, b in tr.members(r, k):
        ca, cb = cov(a), cov(b)
        t, length = ca if ca[1] <= cb[1] else cb
        if length > n // 4:
            return False
        lists[t] = length
    return sum(lists.values()) <= n // 4


def filter_collision(ids, members) -> bool:
    if len(members) < PAIR_FILTER_K:
        return False
    slots = [pair_h12(ids[a], ids[b]) for a, b in members]
    return len(set(slots)) < len(slots)


def filter_false_positive(ids, words, members):
    """The non-member pairs of rewritten words (under 32 ids: the classes that use the table) that
    fall into a member's slot."""
    if len(members) < PAIR_FILTER_K:
        return set()
    slots = {pair_h12(ids[a], ids[b]) for a, b in members}
    mset, out = set(members), set()
    for w in words:
        if 2 <= len(w) < 32 and hits(w, members):
            out |= {p for p in zip(w, w[1:]) if p not in mset and pair_h12(ids[p[0]], ids[p[1]]) in slots}
    return out


# ---------------------------------------------------------------- the directed cases
def adjacent():
    return {b"abcd": 1000, b"ab": 50, b"cd": 20, b"xabcdy": 7, b"cdab": 300}, 300


ADJACENT_ZERO_MERGES = ((b"ab", b"c"), (b"d", b"ab"), (b"x", b"ab"))   # three of the nine


def adjacent3():
    return {b"abcdef": 1000, b"efcdab": 300, b"ab": 50, b"cd": 20, b"ef": 10, b"xabcdefy": 7}, 300


def shared_a():
    return {b"ta": 900, b"te": 800, b"ti": 700, b"to": 600, b"xta": 50, b"xte": 40, b"ytiz": 30,
            b"xtoz": 20}, 300


def shared_b():
    return {b"ae": 900, b"be": 800, b"ce": 700, b"de": 600, b"aex": 50, b"bex": 40, b"zcey": 30,
            b"zdex": 20}, 300


def same_list_case():
    """shared_a, and 10 two-letter words for each second letter: "t" is in 8 words, each of "a",
    "e", "i", "o" in 12, and 8 <= 48 / 4 (a list longer than a quarter of the words is not walked)."""
    counts = dict(shared_a()[0])
    for v in b"aeio":
        for n, c in enumerate(b"bcdfghjklm"):
            counts[bytes([c, v])] = 1 + n % 3
    return counts, 300


MULTI_LENGTHS = (6, 7, 9, 12, 15, 17, 20, 31, 33, 40, 63, 64, 80, 100)
MULTI_MEMBERS = ((b"p", b"q"), (b"r", b"s"), (b"u", b"v"))


def multi_hit():
    """Every word of MULTI_LENGTHS begins with "pq", ends with "uv" and holds "rs"; from 9 ids on
    it holds "pq" twice.  "qr" (count 70 000) is the fourth key and clashes with both (p,q) and
    (r,s), so trip 0 is the three members, whose letters are in some 20 of the 260 words: lists.
    The 240 other words are random over "efgh": their pairs follow, in trips that scan."""
    r = SplitMix64(0x3B17)
    fill = lambda n: bytes(b"efgh"[r.below(4)] for _ in range(n))   # noqa: E731
    counts = {b"pq": 100_000, b"rs": 90_000, b"uv": 80_000, b"qr": 70_000}
    for n, L in enumerate(MULTI_LENGTHS):
        if L < 9:
            w = b"pq" + fill(L - 6) + b"rs" + b"uv"
        else:
            free = L - 8
            f1, f2 = free // 3, free // 3
            w = b"pq" + fill(f1) + b"rs" + fill(f2) + b"pq" + fill(free - f1 - f2) + b"uv"
        assert len(w) == L
        counts[w] = 100 + n
    while len(counts) < 4 + len(MULTI_LENGTHS) + 240:
        w = fill(3 + r.below(22))
        if w not in counts:
            counts[w] = 1 + r.below(5)
    return counts, 420


PAIR_FILTER_MEMBERS = ((b"a", b"b"), (b"y", b"l"), (b"c", b"r"), (b"m", b"n"))


def pair_filter():
    """(a,b) and (y,l) share a slot of the pair table; (a,l) and (y,b), no members, fall into
    (c,r)'s slot, in words that (c,r) rewrites."""
    return {b"ab": 900, b"yl": 800, b"cr": 700, b"mn": 600, b"abyl": 50, b"xylab": 40, b"ybcr": 30,
            b"alcr": 20, b"zmnab": 10, b"crmnylab": 5}, 300


def tie_kept():
    """(c,d) and (A,A) tie at 90 below (a,b): (A,A) ends the batch (a == b) and seeds nothing."""
    return {b"ab": 100, b"cd": 90, b"AA": 90}, 300


def tie_cut_between():
    """(a,b) 100, then (o,p), (m,n), (k,l), (i,j) and (D,m) at 90: (D,m) ends the batch at 5 (its b
    is a member's a) and, tied, seeds (m,n), the third member: the batch is (a,b), (o,p), (m,n)."""
    return {b"ab": 100, b"op": 90, b"Dmn": 90, b"kl": 90, b"ij": 90}, 300


def tie_cut_at_gap():
    """(a,b) 100, (o,p) 95, then (m,n), (k,l), (i,j) and (D,a) at 90: (D,a) seeds the first
    member, above the strict gap below (o,p), so the batch is the two above the tie."""
    return {b"ab": 10, b"Dab": 90, b"op": 95, b"mn": 90, b"kl": 90, b"ij": 90}, 300


def cap():
    return {bytes([0x80 + i, 0xC0 + i]): 5000 - i for i in range(40)}, 256 + 37


def overflow():
    return {bytes([0x80 + i, 0xC0 + j]): 1000 for i in range(64) for j in range(8)}, 256 + 512


CASES = {
    "adjacent": adjacent, "adjacent3": adjacent3, "shared_a": shared_a, "shared_b": shared_b,
    "same_list": same_list_case, "multi_hit": multi_hit, "pair_filter": pair_filter,
    "tie_kept": tie_kept, "tie_cut_between": tie_cut_between, "tie_cut_at_gap": tie_cut_at_gap,
    "cap": cap, "overflow": overflow,
}
# the batch caps (BPE355_BATCH) a case also runs under
EXTRA_BATCH = {"pair_filter": (3,), "cap": (5,)}


@functools.lru_cache(maxsize=None)
def trace(case: str, vocab: int | None = None) -> Trace:
    counts, own = CASES[case]()
    return Trace(counts, own if vocab is None else vocab)


@functools.lru_cache(maxsize=None)
def tie_trace(kind: str) -> Trace:
    """The deep-tie text `kind` of tests/tie_cases.py at its scaled size."""
    import tie_cases
    return Trace(B.base_counts(kind), tie_cases.SCALED_VOCAB)


# ---------------------------------------------------------------- rule (3) is not reached
def random_small_corpus(seed: int):
    """(counts, specials) of the search described in the module docstring."""
    rng = random.Random(seed)
    alpha = rng.choice(["ab", "abc", "a", "aab", "abcd"])
    counts = {}
    for _ in range(rng.randint(1, 6)):
        w = "".join(rng.choice(alpha) for _ in range(rng.randint(2, 12))).encode()
        counts[w] = rng.randint(1, 5)
    specials = ()
    if seed % 2:
        w = rng.choice(sorted(counts)).decode()
        i = rng.randrange(len(w))
        specials = (w[i:i + rng.randint(1, 4)],)
    return counts, specials


def makes_same_bytes_twice(counts, specials) -> bool:
    """Does the reference, trained until no pair is left, merge a pair whose bytes are a token
    already (a byte, an earlier merge's token)?  The specials only drop the words equal to one."""
    _vocab, merges = B.train_counts(counts, 100_000, specials)
    toks = [a + b for a, b in merges]
    return len(set(toks)) != len(toks) or any(len(t) < 2 for t in toks)
