"""CPU: the sparse and large vocab-id inputs (tests/vocab_id_cases.py).  For every case and id
map the oracle on the remapped vocab gives f of the oracle's dense ids, the oracle agrees with
the plain-Python restatement of the reference tokenizer (oracle/cpu_ref.py) where the reference's
id bookkeeping is odd -- one byte string under two ids, a special missing from the vocab, that
special's id taken by another token -- and the inputs still do what they are for.  Everything
here comes from the oracle, oracle/cpu_ref.py and plain Python, nothing from the code under test.

Counted with the oracle over the distinct pre-tokens:

  natural       4763 pre-tokens, 63 656 ids in 133 027 bytes.  31 one-byte words; 102 vocab entries
                of 2..16 bytes, all of one id; words of 2..16 bytes that are no entry: 539, 1135,
                1284, 975 and 692 of 2, 3, 4, 5 and 6 or more ids; 5 words over 16 bytes, all of 6
                or more ids.  With 250 of the 500 ids below T, all 4, 8 and 16 arrangements of ids
                below and at or above T occur among the words of 2, 3 and 4 ids.
  constructed   89 pre-tokens, 88 600 ids in 220 440 bytes (14 chunks of 16 KiB), 286 vocab
                entries.  8 one-byte words; vocab entries: 3 of one id, 4, 5, 6 and 1 of 2, 3, 4
                and 5 ids; other words up to 16 bytes: 12, 12, 11, 4 and 2 of 2, 3, 4, 5 and 7 ids;
                words of 17 bytes and more: 1, 7, 5, 6, 1 and 1 of 1, 2, 3, 4, 5 and 7 ids.
                Pre-token lengths 1-5, 7, 15, 16, 17, 18, 22, 32, 35, 48, 64.  Under edge(T_k)
                each population has the k + 2 arrangements among its words of k ids.

The floors asserted below are what the inputs were written to hold (a word of every population
and id count, five one-byte words, every arrangement), not what was counted.
"""
import functools

import pytest

pytest.importorskip("regex")   # oracle/cpu_ref.py pre-tokenizes with it

import vocab_id_cases as V  # noqa: E402
from oracle import cpu_ref  # noqa: E402
from oracle import oracle  # noqa: E402


@functools.lru_cache(maxsize=None)
def _dense(case_name):
    c = V.CASES[case_name]()
    return oracle.encode(c.vocab, c.merges, c.specials, c.text)


@functools.lru_cache(maxsize=None)
def _word_ids(case_name):
    """{pre-token bytes: its dense ids}, each pre-token encoded on its own by the oracle"""
    c = V.CASES[case_name]()
    out = {}
    for w in oracle.word_counts(c.text.encode("utf-8"), c.specials):
        assert oracle.word_counts(w, []) == {w: 1}     # alone it is still one pre-token
        out[w] = oracle.encode(c.vocab, c.merges, [], w.decode("utf-8"))
    return out


def _by_class(case_name):
    c = V.CASES[case_name]()
    S = c.strings()
    count = {}
    for w, ids in _word_ids(case_name).items():
        key = (V.population(w, S), len(ids))
        count[key] = count.get(key, 0) + 1
    return count


@pytest.mark.parametrize("case_name,map_name", V.all_case_maps())
def test_oracle_commutes_with_id_map(case_name, map_name):
    c = V.CASES[case_name]()
    f = V.id_map(map_name, c)
    assert oracle.encode(V.remap(c, f), c.merges, c.specials, c.text) == [f[i] for i in _dense(case_name)]


def test_maps_are_what_they_say():
    for case_name, make in V.CASES.items():
        c = make()
        n = c.n
        for T in V.STRADDLE_T:
            ids = [V.id_map(f"straddle:{T}", c)[i] for i in range(n)]
            assert sum(i < T for i in ids) == n // 2 and max(ids) < 1 << 32
        top = V.id_map("top", c)
        assert sorted(top[i] for i in range(n)) == list(range((1 << 32) - n, 1 << 32))
        f = V.id_map("bytes_high", c)
        assert all((f[i] >= 1 << 30) == (len(b) == 1) for i, b in c.vocab.items())
        f = V.id_map("merged_high", c)
        assert all((f[i] >= 1 << 31) == (len(b) > 1) for i, b in c.vocab.items())
        used = set(_dense(case_name))
        assert sum(len(c.vocab[i]) == 1 for i in used if i < n) >= 5      # one-byte tokens in use
        assert sum(len(c.vocab[i]) > 1 for i in used if i < n) >= 5       # and longer ones


@pytest.mark.parametrize("map_name", ["dense", "top", "collide"])
def test_oracle_matches_python_restatement(map_name):
    """The reference's bookkeeping (tokenizer.py:18-38) where it is odd: b"cd" and b"z" under two
    ids (the later wins), the missing special's id len(vocab), and under "collide" that id already
    taken by b"cde"."""
    c = V.constructed()
    f = V.id_map(map_name, c)
    vocab = V.remap(c, f)
    text = c.text
    enc = cpu_ref.Encoder(vocab, c.merges, c.specials)
    want = enc.encode(text)
    assert oracle.encode(vocab, c.merges, c.specials, text) == want
    n = c.n
    assert enc.vocab_inv[V.SP_MISSING.encode()] == n and want.count(n) > 0
    cd, z = V.token_id(c, b"cd"), V.token_id(c, b"z")
    first_cd = min(i for i, b in c.vocab.items() if b == b"cd")
    assert first_cd < cd and f[cd] in want and f[first_cd] not in want
    assert z > ord("z") and f[z] in want and f[ord("z")] not in want
    if map_name == "collide":
        cde = V.token_id(c, b"cde")
        assert f[cde] == n == enc.vocab_inv[b"cde"]
        assert text.count(V.SP_MISSING) < want.count(n)   # both strings give the id


def test_constructed_populations():
    c = V.constructed()
    count = _by_class("constructed")
    print(sorted(count.items()))
    for nids in (1, 2, 3, 4, 5, 7):
        assert count.get(("long", nids), 0) >= 1
    for nids in (2, 3, 4, 5):
        assert count.get(("dict", nids), 0) >= 1
        assert count.get(("table", nids), 0) >= 1
    assert count.get(("dict", 1), 0) >= 1 and count.get(("byte", 1), 0) >= 5
    lens = {len(w) for w in _word_ids("constructed")}
    print(sorted(lens))
    assert {1, 15, 16, 17} <= lens and max(lens) <= 300
    n_bytes = len(c.text.encode("utf-8"))
    print(f"{len(_word_ids('constructed'))} pre-tokens, {len(_dense('constructed'))} ids, {n_bytes} bytes, {c.n} entries")
    assert 4 * 16384 < n_bytes <= 300_000
    # merges never produce the several-id dictionary words: each is an entry only
    produced = {a + b for a, b in c.merges}
    S = c.strings()
    for w, ids in _word_ids("constructed").items():
        if V.population(w, S) == "dict" and len(ids) > 1:
            assert w not in produced
    # the specials: one in the vocab, one missing (id len(vocab)), one of one byte
    dense = _dense("constructed")
    assert c.n in dense and V.token_id(c, V.SP_IN_VOCAB.encode()) in dense and ord(V.SP_BYTE) in dense
    assert V.SP_MISSING.encode() not in S and V.SP_IN_VOCAB.encode() in S


@pytest.mark.parametrize("k", [2, 3, 4])
def test_constructed_edge_patterns(k):
    """edge(T_k): all below, all at or above, exactly one at or above in each of the k positions,
    in every population; the ids T_k - 1 and T_k themselves are in use."""
    c = V.constructed()
    T = V.T_OF_NIDS[k]
    f = V.id_map(f"edge:{T}", c)
    seen = V.patterns(_word_ids("constructed"), c.strings(), f, T)
    for pop in ("dict", "table", "long"):
        masks = {m for p, n, m in seen if p == pop and n == k}
        print(pop, k, sorted(masks))
        assert V.edge_masks(k) <= masks
    used = {f[i] for i in _dense("constructed")}
    assert {T - 3, T - 2, T - 1, T, T + 1, T + 2} <= used
    S = c.strings()
    exact = [ids for w, ids in _word_ids("constructed").items() if V.population(w, S) == "dict" and len(ids) == k]
    assert all({f[i] for i in ids} <= {T - 1, T} for ids in exact)


@pytest.mark.parametrize("k", [2, 3, 4])
def test_natural_straddle_patterns(k):
    """straddle(T_k): every arrangement of ids below and at or above T_k among the words of k ids"""
    c = V.natural()
    T = V.T_OF_NIDS[k]
    seen = V.patterns(_word_ids("natural"), c.strings(), V.id_map(f"straddle:{T}", c), T)
    masks = {m for _p, n, m in seen if n == k}
    print(k, sorted(masks))
    assert masks == set(range(1 << k))


def test_natural_populations():
    count = _by_class("natural")
    print(sorted(count.items()))
    assert count.get(("byte", 1), 0) >= 20 and count.get(("dict", 1), 0) >= 50
    for nids in (2, 3, 4, 5, 6):
        assert count.get(("table", nids), 0) >= 100


def test_cut_documents():
    for make in V.CASES.values():
        c = make()
        docs = V.cut_documents(c.text, 40, 5)
        assert 35 <= len(docs) <= 40 and "".join(docs) == c.text and all(docs)
