"""Encode inputs whose vocab ids are sparse and large: tokenizers, texts and id maps that put ids
on both sides of every threshold at which csrc/encode.hip packs a word's ids differently.

How a word's ids travel from k_encode_words to the output depends on the ids' size (make_info,
info_inline_ids, build_dictionary, byte_rec, the LDS cache of k_enc_resolve_c):

  one id             a record kRecDirect | id when id < 2^30 - 1 (one-byte words through byte_rec,
                     one-id dictionary words), else a pending entry and the word table
  dictionary         a vocab entry of 2..16 bytes is kept only if every id of its encoding is
                     below 2^30 - 1, else the word takes the word table
  two ids inline     both < 2^31, else the id pool
  three ids inline   all < 2^20, else the id pool
  four ids inline    all < 2^15, else the id pool
  five or more       the id pool (the dictionary's own pool for a dictionary word)

For any map f on ids, Tokenizer({f(i): b}, merges, sp).encode(text) == [f(i) for i in
Tokenizer({i: b}, merges, sp).encode(text)]: a pre-token's ids depend on its bytes alone.  So a
case is a tokenizer with dense ids 0..n-1, a text, and a set of named maps; the expectation is
the oracle on the remapped vocab, and f applied to the oracle's dense ids.

natural()       the committed corpus_en_500 tokenizer with its special and the fixture corpus.en:
                the word table and the scan's cache for short words of 1..6+ ids.
constructed()   a hand-written tokenizer over a few letters, whose text holds
                  words of 17+ bytes (hashed key, no dictionary) of exactly 1, 2, 3, 4, 5 and 7 ids
                    (doubling chains a -> aa -> ... -> a16, b -> ... -> b16, " " + a16)
                  vocab entries of 2..16 bytes that no merge produces: as pre-tokens they are
                    dictionary words of 2, 3, 4 and 5 ids (over the letters p, q)
                  words of 2..16 bytes that are no vocab entry (word table) of 2, 3, 4, 5, 7 ids
                    (over the letters x, y)
                  pre-tokens of 15, 16 and 17 bytes (kInline is 16)
                  one-byte words; a special in the vocab; a special missing from it (its id is
                  len(vocab)); a one-byte special; b"cd" and b"z" under two ids each (the later
                  one in dict order wins)
                every word over two "atoms" per population in every arrangement of 2, 3 and 4, so
                that edge(T) can put exactly one id at or above T in every position:
                  population   low atom   high atom
                  dictionary   q  T - 1   p  T
                  word table   y  T - 2   x  T + 1
                  17+ bytes    a16 T - 3  b16 T + 2
                The list is repeated (short words 400 times, long ones 120 times) and shuffled:
                220 KB, 14 chunks of 16 KiB.  A few thousand repeats of everything would pass
                the 300 KB the text is to stay under.

Id maps (id_map(name, case)): "dense", "straddle:T" (ids shifted so that about half lie below T),
"top" (the highest n ids), "scatter" (i -> (2654435761 i + 12345) mod 2^32), "bytes_high" (every
one-byte token at 2^30 + id: no one-byte word is direct), "merged_high" (every longer token at
2^31 + id), "edge:T" (constructed case, above), "collide" (constructed case: the token b"cde"
takes the id len(vocab), which the missing special also gets: two byte strings share an id),
"sparse22" (i -> 7919 i + 17, below 2^22: ids the decoder's dense table takes).
The id of a missing special is len(vocab) under every map: maps carry it as n -> n.

patterns() is the coverage helper: tests/test_vocab_id_cases.py asserts on the CPU, with the
oracle alone, that the inputs still reach every class above.
"""
from __future__ import annotations

import functools

import golden_cases as G
import gpt2_files
from synth_text import SplitMix64

T2, T3, T4 = 1 << 31, 1 << 20, 1 << 15      # the inline thresholds of two, three and four ids
T_OF_NIDS = {2: T2, 3: T3, 4: T4}
DIRECT = (1 << 30) - 1                      # kRecPayload: direct ids are below this
STRADDLE_T = (T4, T3, DIRECT, T2)
SCATTER_MUL, SCATTER_ADD = 2654435761, 12345

A16, B16 = "a" * 16, "b" * 16
SP_IN_VOCAB, SP_MISSING, SP_BYTE = "<|eot|>", "<|missing|>", "^"


class Case:
    def __init__(self, name, vocab, merges, specials, text, n_missing=0):
        self.name, self.vocab, self.merges, self.specials, self.text = name, vocab, merges, specials, text
        self.n = len(vocab)                  # dense ids 0..n-1; missing specials get n, n + 1, ...
        self.n_missing = n_missing
        assert list(vocab) == list(range(self.n))

    def strings(self):
        return set(self.vocab.values())


def _arrangements(k, lo, hi, every=False):
    """words of k atoms: all low, all high, exactly one high in each position (every: all 2^k)"""
    if every:
        return ["".join(hi if m >> j & 1 else lo for j in range(k)) for m in range(1 << k)]
    return [lo * k, hi * k] + ["".join(hi if j == i else lo for j in range(k)) for i in range(k)]


def _shuffle(r, items):
    for i in range(len(items) - 1, 0, -1):
        j = r.below(i + 1)
        items[i], items[j] = items[j], items[i]


SHORT_REPEATS, LONG_REPEATS = 400, 120


@functools.lru_cache(maxsize=None)
def constructed() -> Case:
    vocab = {i: bytes([i]) for i in range(256)}
    merges = []

    def merge(a, b):
        merges.append((a.encode(), b.encode()))
        vocab[len(vocab)] = (a + b).encode()

    for c in "ab":                            # c -> cc -> c4 -> c8 -> c16
        for k in (1, 2, 4, 8):
            merge(c * k, c * k)
    merge(" ", A16)                           # " " + a16: a token of 17 bytes
    merge("c", "d")
    merge("cd", "e")
    vocab[len(vocab)] = SP_IN_VOCAB.encode()
    # entries that no merge produces (as pre-tokens: dictionary words of several ids)
    dict_words = (_arrangements(2, "q", "p", True) + _arrangements(3, "q", "p") + _arrangements(4, "q", "p")
                  + ["pqpqp"])
    for w in dict_words:
        vocab[len(vocab)] = w.encode()
    vocab[len(vocab)] = b"cd"                 # a second id for a merged token and for a byte: the
    vocab[len(vocab)] = b"z"                  # later one is the id encode gives
    table_words = (_arrangements(2, "y", "x", True) + _arrangements(3, "y", "x") + _arrangements(4, "y", "x")
                   + ["xyxyx", "xyxyxyx", "a" * 15])
    long_words = (_arrangements(2, A16, B16, True) + _arrangements(3, A16, B16) + _arrangements(4, A16, B16)
                  + [A16 + B16 + "xyz", A16 + "xyzxyz", "a" * 17, "b" * 17])
    bare_short = dict_words + table_words + ["a" * 16, "cd", "cde", "p", "q", "x", "y", "z", "!", "7"]
    spaced_short = ["a" * 14, "a" * 15, "zz", "cd", "cde", "q"]
    short = (["\n" + w for w in bare_short] + [" " + w for w in spaced_short]
             + [SP_IN_VOCAB, SP_MISSING, SP_BYTE, "\n" + SP_IN_VOCAB, " " + SP_MISSING, " " + SP_BYTE])
    long_ = ["\n" + w for w in long_words] + [" " + A16, " " + A16 + "x"]
    items = short * SHORT_REPEATS + long_ * LONG_REPEATS
    _shuffle(SplitMix64(0x1D5CA5E5), items)
    return Case("constructed", vocab, merges, [SP_IN_VOCAB, SP_MISSING, SP_BYTE], "".join(items), n_missing=1)


@functools.lru_cache(maxsize=None)
def natural() -> Case:
    o, vocab, merges = G.train_expect("corpus_en_500")
    text = (gpt2_files.FIXTURES / "corpus.en").read_text(encoding="utf-8")
    return Case("natural", vocab, merges, list(o["special_tokens"]), text)


CASES = {"natural": natural, "constructed": constructed}
COMMON_MAPS = (["dense"] + [f"straddle:{T}" for T in STRADDLE_T]
               + ["top", "scatter", "bytes_high", "merged_high"])
MAPS = {"natural": COMMON_MAPS,
        "constructed": COMMON_MAPS + [f"edge:{T}" for T in (T2, T3, T4)] + ["collide"]}


def all_case_maps():
    return [(c, m) for c in CASES for m in MAPS[c]]


def token_id(case: Case, b: bytes) -> int:
    """the dense id encode gives for the token b: the last one in dict order"""
    return max(i for i, v in case.vocab.items() if v == b)


def id_map(name: str, case: Case) -> dict:
    """dense id -> id, over 0..n-1 and the ids n.. of the missing specials (which stay)"""
    n = case.n
    kind, _, arg = name.partition(":")
    if kind == "dense":
        f = {i: i for i in range(n)}
    elif kind == "straddle":
        T = int(arg)    # n // 2 ids below T: with it every arrangement of ids below and at or above T
        f = {i: T - n // 2 + i for i in range(n)}   # occurs among the natural case's words of 2, 3, 4 ids
    elif kind == "top":
        f = {i: (1 << 32) - n + i for i in range(n)}
    elif kind == "scatter":
        f = {i: (SCATTER_MUL * i + SCATTER_ADD) % (1 << 32) for i in range(n)}
    elif kind == "sparse22":      # sparse, and every id below 2^22: within the decoder's 2^28
        f = {i: 7919 * i + 17 for i in range(n)}
    elif kind == "bytes_high":
        f = {i: (1 << 30) + i if len(b) == 1 else i for i, b in case.vocab.items()}
    elif kind == "merged_high":
        f = {i: (1 << 31) + i if len(b) > 1 else i for i, b in case.vocab.items()}
    elif kind == "edge":
        T = int(arg)
        f = {i: i for i in range(n)}
        for tok, v in ((b"q", T - 1), (b"p", T), (b"y", T - 2), (b"x", T + 1),
                       (A16.encode(), T - 3), (B16.encode(), T + 2)):
            f[token_id(case, tok)] = v
    elif kind == "collide":
        f = {i: i for i in range(n)}
        f[token_id(case, b"cde")] = n
    else:
        raise ValueError(name)
    for k in range(case.n_missing):
        f[n + k] = n + k
    if kind != "collide":
        assert len(set(f.values())) == len(f), f"{name} is not injective on {case.name}"
    assert all(0 <= v < (1 << 32) for v in f.values())
    return f


def remap(case: Case, f: dict) -> dict:
    """the vocab under f, in the same dict order"""
    return {f[i]: b for i, b in case.vocab.items()}


def population(word: bytes, strings) -> str:
    """which way a pre-token of these bytes takes: "byte" (one byte), "dict" (a vocab entry of
    2..16 bytes), "table" (2..16 bytes, no entry), "long" (17 bytes or more: hashed key)"""
    if len(word) == 1:
        return "byte"
    if len(word) > 16:
        return "long"
    return "dict" if word in strings else "table"


def patterns(word_ids: dict, strings, f: dict, T: int) -> set:
    """word_ids: {pre-token bytes: its dense ids}.  -> {(population, nids, bitmask of the
    positions whose id under f is at or above T)}"""
    out = set()
    for w, ids in word_ids.items():
        mask = sum(1 << j for j, i in enumerate(ids) if f[i] >= T)
        out.add((population(w, strings), len(ids), mask))
    return out


def edge_masks(k: int) -> set:
    """all below, all at or above, exactly one at or above in each of the k positions"""
    return {0, (1 << k) - 1} | {1 << j for j in range(k)}


def cut_documents(text: str, n_docs: int, seed: int):
    """the text cut into n_docs documents at arbitrary character positions"""
    r = SplitMix64(seed)
    cuts = sorted({1 + r.below(len(text) - 1) for _ in range(n_docs - 1)})
    return [text[a:b] for a, b in zip([0] + cuts, cuts + [len(text)])]
