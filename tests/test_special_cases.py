"""CPU: the inputs of tests/special_cases.py reach what they claim, by the references alone.

For every case the two references (oracle.cpu_ref.Encoder, the C oracle) agree and the ids decode
back to the text; then, per family, conditions on the case itself: the lengths and twins of the
specials, which side of kSpLds the matched specials lie on, the raw matches per 4 KiB stretch and
in total against kSpBuf and the first capacity of the match list, overlapping raw matches present
or absent, every (before, after) pair, where the placed specials start, and the segments per chunk
window against kSegLds with the exact 64 / 65 pair.  For the training lists: the references agree,
and the lists that drop frequent words change the merges while the others do not.
"""
from __future__ import annotations

import functools

import pytest

import special_cases as S
from oracle import cpu_ref, oracle


@functools.lru_cache(maxsize=None)
def _ids(name):
    c = S.CASES[name]()
    enc = cpu_ref.Encoder(c.vocab, c.merges, c.specials)
    return tuple(tuple(enc.encode(t)) for t in c.texts), enc


def _family(family):
    return [n for n, f in S.CASES.items() if f().family == family]


@pytest.mark.parametrize("name", list(S.CASES))
def test_references_agree_and_round_trip(name):
    c = S.CASES[name]()
    by_python, enc = _ids(name)
    # (a missing special is vocab[bytes] = id in the reference, tokenizer.py:35-38: by vocab_inv)
    token = {i: b for b, i in enc.vocab_inv.items()}
    for text, ids in zip(c.texts, by_python):
        assert list(ids) == oracle.encode(c.vocab, c.merges, c.specials, text)
        assert b"".join(token[i] for i in ids).decode("utf-8") == text
    assert sum(len(t.encode("utf-8")) for t in c.texts) <= 512 * 1024


@pytest.mark.parametrize("name", list(S.CASES))
def test_specials_occur_and_vocab_rule(name):
    """every special is matched somewhere, every near-miss stands in the text; every special is a
    vocab entry, but for the one case that says otherwise, whose lengths all differ"""
    c = S.CASES[name]()
    order = S.library_order(c.specials)
    matched = set()
    for t in c.texts:
        _data, m, _lens = S.case_matches(c, t)
        matched |= {k for _p, k in m}
    assert matched == set(range(len(order)))
    have = set(c.vocab.values())
    if name == "missing":
        assert not any(s.encode("utf-8") in have for s in c.specials)
        assert len({len(s) for s in c.specials}) == len(c.specials)
        assert len({len(s.encode("utf-8")) for s in c.specials}) == len(c.specials)
    else:
        assert all(s.encode("utf-8") in have for s in c.specials)
    if c.family in ("lengths", "many", "missing"):
        joined = "".join(c.texts)
        for s in c.specials:
            if len(s) > 1:
                assert s[:-1] in joined.replace(s, "")
            assert S.last_changed(s).encode("utf-8")[:-1] == s.encode("utf-8")[:-1]   # all but the last byte
            assert S.last_changed(s) in joined


def test_merges_give_one_id_and_several_id_words():
    c = S.many()
    enc = cpu_ref.Encoder(c.vocab, c.merges, c.specials)
    n_ids = {w: len(enc.encode(w)) for w in S.FILL}
    assert {n_ids[w] for w in (" the", "'s", "'ll", "é", "  ", "\n\n", "12", "abc")} == {1}
    assert all(n_ids[w] > 1 for w in (" cat", " xyz", " naïve", "東京", " 1234"))
    for w in S.FILL:
        assert w in c.text


# ---------------------------------------------------------------------- lengths
@pytest.mark.parametrize("name", _family("lengths"))
def test_lengths_and_twins(name):
    c = S.CASES[name]()
    by_len = c.claims["by_len"]
    want = [L for L in S.LENGTHS if not (name == "lengths_utf8" and L == 1)]
    assert list(by_len) == want and 1100 > S.K_HALO
    assert len(S.library_order(c.specials)) <= S.K_SP_LDS          # every one under the LDS masks
    for L, group in by_len.items():
        b = [s.encode("utf-8") for s in group]
        assert all(len(x) == L for x in b)
        if L < S.TWIN_FROM:
            assert len(group) == 1
            continue
        assert len(group) == (2 if L == 17 else 3)
        assert all(x[:16] == b[0][:16] for x in b)
        assert b[1][16] != b[0][16] or L > 17 and b[1][:19] != b[0][:19]   # differs where the tail begins
        assert b[-1][:-1] == b[0][:-1] and b[-1][-1] != b[0][-1]           # differs in the last byte only
    firsts = {s.encode("utf-8")[0] for s in c.specials}
    if name == "lengths_utf8":
        assert all(f >= 0x80 for f in firsts) and {f >> 5 for f in firsts} == {6, 7}   # bitmap words 6, 7
        assert all(any(len(ch.encode("utf-8")) == k for ch in "".join(c.specials)) for k in (2, 3))
    else:
        assert all(s.isascii() for s in c.specials)
    _data, m, lens = S.case_matches(c)
    assert not S.has_overlap(m, lens)                                # the device builds the segments


def test_many_specials_on_both_sides_of_the_lds_copies():
    c = S.many()
    order = S.library_order(c.specials)
    lens = S.special_lengths(c.specials)
    assert len(order) >= 130
    assert min(lens[:S.K_SP_LDS]) > max(lens[S.K_SP_LDS + 6:])     # the later ones are the short ones
    assert {1, 2, 3} <= set(lens[S.K_SP_LDS:])
    _data, m, _lens = S.case_matches(c)
    hit = {k for _p, k in m}
    assert hit == set(range(len(order)))                            # both groups, every member
    assert not S.has_overlap(m, lens)
    given = c.specials
    assert given != order and sorted(given) == sorted(order)        # the library has to sort them


# ---------------------------------------------------------------------- dense
@pytest.mark.parametrize("name", _family("dense"))
@pytest.mark.parametrize("lead", [0, 1, 3, 8, 15])
def test_dense_overflows_the_staging_buffer(name, lead):
    """lead: the text's first byte that far past a 16-byte boundary (the unaligned-pointer runs)"""
    c = S.CASES[name]()
    data, m, lens = S.case_matches(c)
    per = S.stretch_counts(m, lead)
    assert sum(1 for v in per.values() if v > S.K_SP_BUF) >= 3
    assert any(0 < v <= S.K_SP_BUF for v in per.values())
    assert len(m) > S.match_capacity(len(data)) > 1024              # the n / 64 term, and the second launch
    assert S.has_overlap(m, lens) == c.claims["overlaps"]
    if c.claims["overlaps"]:                                        # a special and its prefix at one position
        both = len(m) - len({p for p, _k in m})                     # positions that hold the two
        assert both > 3 * S.K_SP_BUF and both * 2 > 0.9 * len(m)
    else:
        assert lens == [1]


# ---------------------------------------------------------------------- overlap
def test_overlap_kinds_present():
    c = S.overlap()
    data, m, lens = S.case_matches(c)
    order = S.library_order(c.specials)
    at = {}
    for p, k in m:
        at.setdefault(order[k], []).append(p)

    def overlaps(x, y):
        """an occurrence of y begins inside an occurrence of x, or at the same byte when x != y"""
        ends = {p: p + len(x.encode()) for p in at[x]}
        ys = set(at[y])
        return any(q in ys for p, e in ends.items() for q in range(p if x != y else p + 1, e))

    for x, y in (("aa", "aa"), ("aba", "aba"), ("ab", "bc"), ("a b", "b c"), ("<|a|>", "<|a|"),
                 ("<|a|", "<|a"), ("<|a", "<"), (S.EOT + S.EOT, S.EOT), (S.EOT, S.EOT + S.EOT)):
        assert overlaps(x, y), (x, y)
    text = c.text
    for k in range(1, 10):                                           # runs of a of every length 1..9
        assert any(text[i:i + k + 2][1:-1] == "a" * k and text[i] not in "ab" and text[i + k + 1] not in "ab"
                   for i in range(len(text) - k - 1)), k
    assert S.has_overlap(m, lens)
    # what re.split keeps differs from the raw list: leftmost-longest had something to decide
    assert len(S.segments(len(data), m, lens)) < 2 * len(m)


def test_overlap_twin_has_none():
    c, t = S.overlap(), S.overlap_twin()
    assert t.text == c.text and set(t.specials) < set(c.specials)
    _data, m, lens = S.case_matches(t)
    assert len(m) > 500 and not S.has_overlap(m, lens)


def test_overlap_safe_split_points_inside_specials():
    """a U+0020 between ASCII non-space bytes inside "a b" / "b c": where encode over several
    ranks would like to cut"""
    data, m, lens = S.case_matches(S.overlap())
    order = S.library_order(S.OVERLAP_SPECIALS)
    inside = [p + 1 for p, k in m if order[k] in ("a b", "b c")]
    assert len(inside) > 1000
    assert all(S.safe_split(data, q) == q for q in inside)
    for ranks in (2, 3, 5):      # a slab boundary whose first safe point lies inside a special
        assert S.spanned_first_cuts(data, m, lens, ranks) >= 1, ranks
    assert S.safe_split(b"ab cd", 4) == 2 and S.safe_split(b"ab  cd", 5) == 0 and S.safe_split(b"a b", 2) == 1


# ---------------------------------------------------------------------- context
def test_context_every_pair():
    product = {(b, a) for b in S.BEFORE for a in S.AFTER}
    each = S.context_each()
    assert len(each.texts) == len(product) == 99
    assert [S.context_pairs([t]) >= {pair} for t, pair in
            zip(each.texts, [(b, a) for b in S.BEFORE for a in S.AFTER])] == [True] * 99
    assert S.context_pairs(each.texts) >= product
    joined = S.context_joined()
    assert len(joined.texts) == 1
    inner = {(b, a) for b, a in product if b != "start" and a != "end"}
    assert S.context_pairs(joined.texts) >= inner
    assert joined.text.startswith(S.CTX) and joined.text.endswith(S.CTX_OTHER)


# ---------------------------------------------------------------------- placement
def test_placement_offsets():
    c = S.placement()
    data, m, lens = S.case_matches(c)
    order = S.library_order(c.specials)
    found = {(order[k], p) for p, k in m}
    at = c.claims["at"]
    assert found == {(sp, p) for _what, sp, p in at}
    assert sorted(lens) == [13, 200]
    for sp in c.specials:
        L = len(sp)
        mine = {what: p for what, s, p in at if s == sp}
        assert [mine[f"block+{o}"] % S.BLOCK for o in S.BLOCK_OFFSETS] == [0, 1, 62, 63, 0]
        for d in (1, 7, 13):
            assert mine[f"boundary-{d}"] % S.K_CHUNK == S.K_CHUNK - d
        assert mine["boundary-0"] % S.K_CHUNK == 0
        assert (mine["ends-on-boundary"] + L) % S.K_CHUNK == 0
        h = mine["halo-end"] % S.K_CHUNK                             # in the halo of the chunk before
        assert S.K_HALO - 16 <= h < S.K_HALO and h + L > S.K_HALO + S.K_POST or L == 13 and h + L > S.K_HALO
    assert len(data) > 12 * S.K_CHUNK


# ---------------------------------------------------------------------- segments per chunk
def _windows(name):
    c = S.CASES[name]()
    data, m, lens = S.case_matches(c)
    assert not S.has_overlap(m, lens)
    return S.window_segment_counts(len(data), S.segments(len(data), m, lens))


def test_segments_per_chunk_window():
    few, many_ = _windows("seg_few"), _windows("seg_many")
    assert len(few) >= 3 and max(few) <= S.K_SEG_LDS and min(few[:3]) > 20
    assert max(many_) > 10 * S.K_SEG_LDS and min(many_[:3]) <= S.K_SEG_LDS    # both ways in one text
    w64, w65 = _windows("seg_64"), _windows("seg_65")
    assert w64[1] == S.K_SEG_LDS == S.seg_64().claims["window1"]
    assert w65[1] == S.K_SEG_LDS + 1 == S.seg_65().claims["window1"]
    a, b = S.seg_64().text, S.seg_65().text
    assert len(a) == len(b)
    diff = [i for i in range(len(a)) if a[i] != b[i]]
    assert diff and b[diff[0]:diff[0] + 13] == S.EOT and diff[-1] - diff[0] < 13   # one special apart
    assert b.count(S.EOT) == a.count(S.EOT) + 1
    assert S.window_segment_counts(3 * S.K_CHUNK, [(0, 10, -1), (10, 3 * S.K_CHUNK, -1)]) == [2, 1, 1]


def test_helpers_on_a_small_example():
    sp = ["b", "abc", "ab", "ab", "éa"]
    assert S.library_order(sp) == ["abc", "éa", "ab", "b"]
    data = "xabcab éab".encode("utf-8")
    m = S.raw_matches(data, sp)
    assert m == [(1, 0), (1, 2), (2, 3), (4, 2), (5, 3), (7, 1), (9, 2), (10, 3)]
    lens = S.special_lengths(sp)
    assert lens == [3, 3, 2, 1] and S.has_overlap(m, lens)
    assert S.segments(len(data), m, lens) == [(0, 1, -1), (1, 4, 0), (4, 6, 2), (6, 7, -1), (7, 10, 1), (10, 11, 3)]
    assert S.stretch_counts([(0, 0), (4095, 0), (4096, 0)], 0) == {0: 2, 1: 1}
    assert S.stretch_counts([(0, 0), (4095, 0), (4096, 0)], 1) == {0: 1, 1: 2}
    assert S.match_capacity(1000) == 1024 and S.match_capacity(1 << 20) == 16384


# ---------------------------------------------------------------------- training lists
@functools.lru_cache(maxsize=None)
def _trained(name):
    vocab, merges, _info = cpu_ref.train(S.train_corpus(), S.TRAIN_VOCAB, S.TRAIN_LISTS[name][0])
    return vocab, merges


def test_train_corpus_holds_the_words():
    text = S.train_corpus()
    assert 150_000 < len(text.encode("utf-8")) < 320_000
    counts = cpu_ref.count_pretokens(text, [])
    for w in list(S.WORDS.values()) + S.OTHER_WORDS + S.SIXTY:
        assert counts.get(w, 0) >= 20, w
    assert sorted(map(len, S.WORDS.values())) == [2, 7, 8, 16, 17, 40]
    for s in S.TRAIN_LISTS["never"][0] + S.TRAIN_LISTS["no_pretoken"][0] + S.TRAIN_LISTS["merge_products"][0]:
        assert s not in counts
    assert S.EOT in text and "the cat" in text


@pytest.mark.parametrize("name", list(S.TRAIN_LISTS))
def test_train_lists(name):
    specials, matters = S.TRAIN_LISTS[name]
    vocab, merges = _trained(name)
    assert (vocab, merges) == oracle.train_raw(S.train_corpus().encode("utf-8"), S.TRAIN_VOCAB, specials)
    _v0, without = _trained("none")
    slots = len({s for s in specials if len(s.encode("utf-8")) > 1})
    assert len(merges) == S.TRAIN_VOCAB - 256 - slots               # a one-byte special takes no slot
    # a filter that did nothing would choose the merges of "none", as many as there is room for
    assert (merges != without[:len(merges)]) == matters
    products = {a + b for a, b in merges}
    taken = [s for s in dict.fromkeys(specials) if s.encode("utf-8") in products]
    assert len(vocab) == S.TRAIN_VOCAB - len(taken)                  # add_token adds nothing for those
    if name == "merge_products":
        assert len(taken) >= 2 and "th" in taken
    if name == "duplicates":
        assert len(set(specials)) < len(specials)
    if name == "seventy":
        assert len(set(specials)) == 70
