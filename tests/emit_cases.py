"""Encode inputs built for the thresholds of the id emit (k_enc_emit, k_enc_cut_offsets) and of the
word loads in front of it (load_word, enc_table_add) in csrc/encode.hip.

The emit handles PARTS: K_EMIT_PARTS per 16 KiB chunk.  A chunk's mc records (one per pre-token
whose FIRST byte lies in the chunk, a special token one record) are split at r0 = mc * part //
K_EMIT_PARTS, and a part of m records and T ids takes one of three write paths:

  (a)  m <= PART_RECORDS (2048) and T <= K_EMIT_IDS (6144): the ids staged in LDS, stored as a
       scalar head up to 16-byte alignment of out + P, a body of 16-byte stores (uint16: packed
       pairs) and a scalar tail
  (b)  m <= 2048 and T > 6144: straight to memory
  (c)  m > 2048: rounds of 256 records with a running offset

plan() restates that split in plain Python from the oracle's pre-tokens and per-word id counts;
tests/test_emit_cases.py shows on the CPU that every case below holds the parts it is built for.
P is a part's first id position (the exclusive sum of the Ts) and head(e) the scalar head's
length for ids of e bytes.  head() assumes that the output's base address is 16-byte aligned,
which holds for the device buffers the library and torch allocate.

The tokenizer is hand-made so that a word's id count is arithmetic:
  x y z          no merge: " " + L - 1 such letters is a word of L bytes and L ids (xword)
  "ab"           one id; " a", " ab" one id; a tail of b times "ab" takes b ids off a word
  gh doubling    "gh", "ghgh", ("gh")^4, ("gh")^8 (GH16, 16 bytes) one id each, and each with a
                 leading space one id: one-id words of 3, 5, 9 and 17 bytes (ONE)
  jk chain       JK15 = ("jk")^7 "j", a vocab entry of 15 bytes
  <|endoftext|>  the special
wide_vocab() is the same tokenizer with the byte "w" under id 70 000 and every other id below
65 536, for the uint16 refusals.

Cases (each a function returning text; all ASCII, no "\\r"):
  path_a_edges   one chunk per probe: a long x-word, then 2 T - 1 one-id words, so that part 1 is
                 T one-id records; the long word's "ab" tail sets P mod 8.  T = head - 1, head,
                 head + 1, head + kPer at every residue of both widths; T = 0 (a one-record
                 chunk), 1, 6143, 6144
  path_b         few records and T = 6145, 10 239, 10 240, 16 384 (one word), 6144 / 6145 by one
                 byte; 2048 records and T = 6145
  records_edge   parts of m = 2047, 2048, 2049, 4096 and 8192 records, one- and several-id
  empty_chunks   a 40 KiB word (two chunks without a record), a special and a word as a chunk's
                 only record, a last chunk of 6 bytes
  mixed_reuse    a block of 3 chunks + 8 bytes holding every path, repeated: every repetition
                 meets the chunk grid at another phase
  word_loads     every word length 1..40 at every byte alignment, near-twins of 15, 16, 17 bytes,
                 long twins, NUL words, vocab entries; word_load_tails(): short texts whose last
                 word of 1..40 bytes has 0..24 bytes after it
  refusal_*      one wide id in a head element, a packed pair's even and odd slot, a tail
                 element, a path-(b) part and a path-(c) part's first and later rounds
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import oracle

# restated from csrc/stage.h and csrc/encode.hip (tests/test_emit_cases.py reads the source)
K_CHUNK = 16384
K_EMIT_PARTS = 2
K_EMIT_IDS = 12288 // K_EMIT_PARTS
K_EMIT_R = 16 // K_EMIT_PARTS
K_CUT_ROUND = 256 * K_EMIT_R
K_ENC_INLINE = 15
K_INLINE = 16
SOURCE_CONSTANTS = {
    "K_CHUNK": ("stage.h", "kChunk"), "K_INLINE": ("stage.h", "kInline"),
    "K_EMIT_PARTS": ("encode.hip", "kEmitParts"), "K_EMIT_IDS": ("encode.hip", "kEmitIds"),
    "K_EMIT_R": ("encode.hip", "kEmitR"), "K_CUT_ROUND": ("encode.hip", "kCutRound"),
    "K_ENC_INLINE": ("encode.hip", "kEncInline"),
}
PART_RECORDS = 256 * K_EMIT_R     # a part of more records takes path (c)
ROUND_C = 256                     # records per round of path (c)

EOT = "<|endoftext|>"
SPECIALS = [EOT]
WIDE_BYTE, WIDE_ID = "w", 70_000
GH16 = "gh" * 8
JK15 = "jk" * 7 + "j"


# ---------------------------------------------------------------------- the tokenizer
@functools.lru_cache(maxsize=None)
def _tokenizer():
    vocab = {i: bytes([i]) for i in range(256)}
    merges = []

    def merge(a, b):
        merges.append((a.encode(), b.encode()))
        vocab[len(vocab)] = (a + b).encode()

    merge("a", "b")
    merge("g", "h")
    for k in (1, 2, 4):
        merge("gh" * k, "gh" * k)                                        # ghgh, (gh)^4, GH16
    merge("j", "k")
    merge("jk", "jk")
    merge("jk" * 2, "jk" * 2)
    merge("jk" * 4, "jk" * 2)
    merge("jk" * 6, "jk")
    merge("jk" * 7, "j")                                                 # JK15
    merge(" ", "a")
    merge(" ", "ab")
    for k in (1, 2, 4, 8):
        merge(" ", "gh" * k)
    vocab[len(vocab)] = EOT.encode()
    return vocab, merges


def vocab():
    return dict(_tokenizer()[0])


def merges():
    return list(_tokenizer()[1])


def wide_vocab():
    """the same byte strings; the byte "w" under WIDE_ID, every other id as in vocab()"""
    v = vocab()
    del v[ord(WIDE_BYTE)]
    v[WIDE_ID] = WIDE_BYTE.encode()
    return v


_NIDS: dict = {}


def word_ids(word: bytes) -> int:
    """how many ids the oracle gives the pre-token `word`"""
    n = _NIDS.get(word)
    if n is None:
        v, m = _tokenizer()
        n = _NIDS[word] = len(oracle.encode(v, m, [], word.decode("utf-8")))
    return n


# ---------------------------------------------------------------------- the plan
def records(data: bytes, cuts=()):
    """(starts, lengths, id counts) of the records k_enc_scan4 leaves: the oracle's pre-tokens of
    every stretch between document starts (`cuts`, byte offsets) and specials, a special one
    record of one id"""
    sp = EOT.encode()
    bounds = [0] + sorted({int(c) for c in cuts if 0 < c < len(data)}) + [len(data)]
    starts, lens, nids = [], [], []
    for a, b in zip(bounds, bounds[1:]):
        p = a
        while p < b:
            q = data.find(sp, p, b)
            e = q if q >= 0 else b
            if e > p:
                for s, ln in oracle.pretokenize(data[p:e]):
                    starts.append(p + s)
                    lens.append(ln)
                    nids.append(word_ids(data[p + s:p + s + ln]))
            if q >= 0:
                starts.append(q)
                lens.append(len(sp))
                nids.append(1)
                p = q + len(sp)
            else:
                p = b
    return np.array(starts, dtype=np.int64), np.array(lens, dtype=np.int64), np.array(nids, dtype=np.int64)


class Plan:
    """per chunk mc; per part (index chunk * K_EMIT_PARTS + part) lo (its first record's index in
    the whole text), m, T and P, as k_enc_emit derives them"""

    def __init__(self, starts, nids, n_bytes):
        self.starts, self.nids, self.n_bytes = starts, nids, n_bytes
        n_chunks = (n_bytes + K_CHUNK - 1) // K_CHUNK
        self.mc = np.bincount(starts // K_CHUNK, minlength=n_chunks).astype(np.int64)
        base = np.concatenate([[0], np.cumsum(self.mc)[:-1]])
        part = np.arange(K_EMIT_PARTS)
        self.lo = (base[:, None] + self.mc[:, None] * part // K_EMIT_PARTS).ravel()
        hi = (base[:, None] + self.mc[:, None] * (part + 1) // K_EMIT_PARTS).ravel()
        self.m = hi - self.lo
        self.cs = np.concatenate([[0], np.cumsum(nids)])
        self.P = self.cs[self.lo]
        self.T = self.cs[hi] - self.P

    def drop_records(self):
        """keep the per-part arrays alone (path, head, chunks, locate): for plans of many records"""
        self.starts = self.nids = self.cs = self.lo = None

    def path(self):
        """per part: "a", "b" or "c" """
        return np.where(self.m > PART_RECORDS, "c", np.where(self.T > K_EMIT_IDS, "b", "a"))

    def head(self, e: int):
        """per part: the ids of the scalar head for ids of e bytes (16-byte-aligned output base)"""
        return ((16 - (self.P * e) % 16) % 16) // e

    def chunks(self):
        """[(mc, [(m, T) per part])] per chunk"""
        k = K_EMIT_PARTS
        return [(int(self.mc[c]), [(int(self.m[c * k + p]), int(self.T[c * k + p])) for p in range(k)])
                for c in range(len(self.mc))]

    def locate(self, id_index: int) -> str:
        """the chunk, part and path that holds the id at `id_index`, for failure messages"""
        live = np.flatnonzero(self.T > 0)
        if live.size == 0:
            return "no part holds an id"
        j = int(live[max(int(np.searchsorted(self.P[live], id_index, "right")) - 1, 0)])
        return (f"chunk {j // K_EMIT_PARTS} part {j % K_EMIT_PARTS} path ({self.path()[j]}): m {int(self.m[j])}, "
                f"T {int(self.T[j])}, P {int(self.P[j])}, id {id_index - int(self.P[j])} of the part")

    def region(self, id_index: int, e: int) -> str:
        """where k_enc_emit stores the id at id_index for ids of e bytes: "head", "body0" .. (the
        slot in its 16-byte store), "tail", "b", "c<round>" """
        j = int(np.searchsorted(self.P, id_index, "right")) - 1
        while self.T[j] == 0:
            j -= 1
        q, path = id_index - int(self.P[j]), self.path()[j]
        assert 0 <= q < self.T[j]
        if path == "b":
            return "b"
        if path == "c":
            r = int(np.searchsorted(self.cs, id_index, "right")) - 1 - int(self.lo[j])   # the record in the part
            return f"c{r // ROUND_C}"
        per, T = 16 // e, int(self.T[j])
        h = min(int(self.head(e)[j]), T)
        body = (T - h) // per
        if q < h:
            return "head"
        if q < h + per * body:
            return f"body{(q - h) % per}"
        return "tail"

    def id_index(self, data: bytes, pos: int) -> int:
        """the index of the id that the byte at `pos` becomes, for a byte no merge touches"""
        j = int(np.searchsorted(self.starts, pos, "right")) - 1
        k = pos - int(self.starts[j])
        return int(self.cs[j]) + (word_ids(data[int(self.starts[j]):pos]) if k else 0)


def plan_of(text: str, cuts=()) -> Plan:
    data = text.encode("utf-8")
    starts, _lens, nids = records(data, cuts)
    return Plan(starts, nids, len(data))


def plan(text: str):
    """[(mc, [(m, T) per part])] per chunk"""
    return plan_of(text).chunks()


# ---------------------------------------------------------------------- words
ONE = {2: " a", 3: " ab", 5: " ghgh", 9: " " + "gh" * 4, 17: " " + GH16}   # one record, one id, by byte length


def xword(n_bytes: int, b: int = 0, phase: int = 0) -> str:
    """one word of n_bytes bytes and n_bytes - b ids: a space, unmerged letters, b times "ab" """
    k = n_bytes - 1 - 2 * b
    assert k >= 1 and b >= 0
    return " " + ("xyz" * (k // 3 + 2))[phase % 3:phase % 3 + k] + "ab" * b


_FILL = [" ab", " xyz", " a", " ghgh", " abab", " " + GH16, " x", " " + "gh" * 4, " ab", " zyx", " " + JK15, " abx"]


class _Text:
    def __init__(self):
        self.parts, self.n, self.k = [], 0, 0

    def add(self, s: str):
        self.parts.append(s)
        self.n += len(s)

    def fill_to(self, end: int):
        """ordinary short words up to byte `end` exactly"""
        assert end - self.n >= 2
        while end - self.n >= 32:
            self.add(_FILL[self.k % len(_FILL)])
            self.k += 1
        self.add(xword(end - self.n, 0, self.k))

    def text(self) -> str:
        return "".join(self.parts)


def _probe_small(T: int, phase: int) -> str:
    sizes = (3, 2, 5, 3, 9, 3, 17)
    return "".join(ONE[sizes[(i + phase) % len(sizes)]] for i in range(max(2 * T - 1, 0)))


def _probe_chunk(T: int, b: int, phase: int) -> str:
    """one chunk: a long word, then 2 T - 1 one-id words -- mc = 2 T, part 1 is T one-id records
    (T = 0: the long word alone, mc = 1, part 0 empty)"""
    small = _probe_small(T, phase)
    return xword(K_CHUNK - len(small), b, phase) + small


def a_edge_targets():
    """(residue of P mod 8, T) of the probes: for uint16 every residue r with T = head - 1, head,
    head + 1, head + 8; for uint32 every residue mod 4 with T = head - 1, head, head + 1, head + 4,
    placed at the residue mod 8 where the uint16 list has that T already if there is one"""
    want = []
    for r in range(8):
        h = (8 - r) % 8
        want += [(r, T) for T in (h - 1, h, h + 1, h + 8) if T >= 1]
    for r4 in range(4):
        h = (4 - r4) % 4
        for T in (h - 1, h, h + 1, h + 4):
            if T >= 1 and (r4, T) not in want and (r4 + 4, T) not in want:
                want.append((r4, T))
    return want


def _dense_chunk(part0, part1) -> str:
    """a chunk of exactly the given records, part 0 then part 1"""
    assert len(part1) - len(part0) in (0, 1)
    s = "".join(part0) + "".join(part1)
    assert len(s) == K_CHUNK, len(s)
    return s


def _chunk_6144():
    return _dense_chunk([" xy"] * 2048, [" ghgh"] * 2048)                            # T 6144 | 2048


def _chunk_6143():
    return _dense_chunk([" xy"] * 2047 + [" x"], [" ghgh"] * 2047 + [" ababa"])       # T 6143 | 2050


def _chunk_6145():
    return _dense_chunk([" xy"] * 2047 + [" xyz"], [" ghgh"] * 2047 + [" aba"])       # T 6145 (b, m 2048) | 2049


@functools.lru_cache(maxsize=None)
def path_a_edges() -> str:
    out, P = [], 0
    empty_at = {0, 7}     # T = 0 is T = head at P = 0 and T = head - 1 at P = 7 (mod 8; mod 4: 0 and 3)
    for i, (r, T) in enumerate([(0, 0)] + a_edge_targets()):
        if P % 8 in empty_at:                             # a one-record chunk: part 0 is empty at this P
            empty_at.discard(P % 8)
            out.append(_probe_chunk(0, 0, i))
            P += K_CHUNK
        if T == 0:
            continue
        long_bytes = K_CHUNK - len(_probe_small(T, i))
        b = (P + long_bytes + T - 1 - r) % 8              # part 1 begins at P + (long_bytes - b) + T - 1
        out.append(_probe_chunk(T, b, i))
        P += long_bytes - b + 2 * T - 1
    assert not empty_at
    out += [_chunk_6143(), _chunk_6144()]
    return "".join(out)


@functools.lru_cache(maxsize=None)
def path_b() -> str:
    def words(sizes, b=0):
        return [xword(n, b if i == 1 else 0, i) for i, n in enumerate(sizes)]
    return "".join([
        _dense_chunk(words([1536] * 4), words([2560] * 4)),                          # T 6144 (a) | 10 240 (b)
        _dense_chunk(words([1536, 1536, 1537, 1536]), words([2560, 2560, 2559, 2560])),   # T 6145 (b) | 10 239
        xword(K_CHUNK, 0, 1),                                                        # mc 1: T 0 | 16 384, m 1
        _chunk_6145(),
        _dense_chunk(words([2048] * 4, 5), words([2048] * 4, 7)),                    # T 8187 | 8185
        _chunk_6144(),
    ])


@functools.lru_cache(maxsize=None)
def records_edge() -> str:
    one_byte = "".join("xyz"[(7 * i) % 3] + "0123456789"[(3 * i) % 10] for i in range(K_CHUNK // 2))
    two = [" x", " a", " z", " a", " y"]                          # 2, 1, 2, 1, 2 ids
    four = [" aba", " xab", " abx", " gha", " xab"]               # 2, 3, 2, 2, 3 ids

    def of(words, n):
        return [words[i % len(words)] for i in range(n)]
    return "".join([
        one_byte,                                                                    # m 8192 | 8192, one id each
        "".join(of(two, 8192)),                                                      # m 4096 | 4096, 1 and 2 ids
        _dense_chunk(of(four, 2048), of(four, 2048)),                                # m 2048 | 2048 (a)
        _dense_chunk(of(four, 2048), of(four, 2047) + [" a", " x"]),                 # m 2048 | 2049
        _dense_chunk(of(four, 2047), of(four, 2047) + [" abababa"]),                 # m 2047 | 2048
        _dense_chunk([" xyz"] * 2048, [" zyx"] * 2048),                              # m 2048 | 2048 (b), T 8192
        _dense_chunk(of(four, 2047) + [" a", " x"], of(four, 2047) + [" x", " a"]),  # m 2049 | 2049, several ids
    ])


LONG_WORD = 40 * 1024


@functools.lru_cache(maxsize=None)
def empty_chunks() -> str:
    t = _Text()
    t.fill_to(16000)
    t.add(xword(LONG_WORD, 3))                       # ends at 56 960: chunks 1 and 2 hold no record
    t.fill_to(4 * K_CHUNK - 10)
    t.add(xword(10 + K_CHUNK - len(EOT), 1))         # runs through chunk 4 up to the special
    t.add(EOT)                                       # chunk 4: the special is its only record
    assert t.n == 5 * K_CHUNK
    t.fill_to(6 * K_CHUNK - 40)
    t.add(xword(40 + K_CHUNK - 3, 2))
    t.add(" ab")                                     # chunk 6: one word is its only record
    assert t.n == 7 * K_CHUNK
    t.add(" ab ab")                                  # chunk 7: 6 bytes
    return t.text()


# ---------------------------------------------------------------------- workgroup reuse
BLOCK_BYTES = 3 * K_CHUNK + 8
NOMINAL_CUS = 256      # an MI355X
MAX_WG_PER_CU = 8      # workgroups of 256 threads a CU holds at most


@functools.lru_cache(maxsize=None)
def reuse_block() -> str:
    """ordinary words (K_CHUNK + 8 bytes), eight words of 2048 bytes, K_CHUNK one-byte pre-tokens;
    begins with " a" and ends with a letter after a digit, so the seam between two blocks is a
    safe split point"""
    t = _Text()
    t.fill_to(K_CHUNK + 8)
    for i in range(8):
        t.add(xword(2048, i % 4, i))
    t.add("".join("0123456789"[(7 * i) % 10] + "xyz"[(5 * i) % 3] for i in range(K_CHUNK // 2)))
    assert t.n == BLOCK_BYTES
    return t.text()


def reuse_parts_needed(cus: int) -> int:
    """1.25 times the most workgroups the emit's launch can ask for: 8 per CU, times its factor 2"""
    return -(-5 * MAX_WG_PER_CU * cus * 2 // 4)


def reuse_reps(cus: int) -> int:
    chunks = -(-reuse_parts_needed(cus) // K_EMIT_PARTS)
    return -(-chunks * K_CHUNK // BLOCK_BYTES)


def mixed_reuse(reps: int) -> str:
    return reuse_block() * reps


def reuse_plan(reps: int) -> Plan:
    """the plan of mixed_reuse(reps), from one block's records (the seam is a safe split point:
    tests/test_emit_cases.py holds the tiling against the records of two blocks)"""
    starts, _lens, nids = records(reuse_block().encode())
    all_starts = (starts[None, :] + BLOCK_BYTES * np.arange(reps, dtype=np.int64)[:, None]).ravel()
    return Plan(all_starts, np.tile(nids, reps), BLOCK_BYTES * reps)


# ---------------------------------------------------------------------- word loads
WORD_LENGTHS = tuple(range(1, 41))
TAIL_LENGTHS = WORD_LENGTHS
TAIL_DISTANCES = tuple(range(0, 25))
_LETTERS = "xyzabqxzyb"


def _word(L: int, seed: int) -> str:
    return "".join(_LETTERS[(seed + 3 * i + i * i) % len(_LETTERS)] for i in range(L))


def _twins():
    """near-twins of 15, 16 and 17 bytes: another byte 0, byte 7, byte 8, last byte; the same
    bytes at the three lengths; longer twins that differ in the last byte alone"""
    base = "zyxzyxzyxzyxzyxzyxzyx"
    out = []
    for L in (K_ENC_INLINE, K_INLINE, K_INLINE + 1):
        w = base[:L]
        out.append(w)
        for k in (0, 7, 8, L - 1):
            out.append(w[:k] + "q" + w[k + 1:])
    for L in (17, 18, 24, 25, 33, 40):
        w = _word(L, 5)
        out += [w[:-1] + "x", w[:-1] + "y"]
    return out


def vocab_entry_words():
    """pre-tokens that are vocab entries of 2..17 bytes"""
    return ["ab", "gh", "ghgh", "gh" * 4, GH16, JK15, " " + GH16, " ab", "jk" * 7, "jk" * 4]


def near_entry_words():
    """no vocab entries, one byte or one length off those"""
    return [GH16[:-1], GH16[:-1] + "g", GH16 + "g", JK15[:-1], JK15[:-1] + "k", JK15 + "j", "gh" * 7 + "gg"]


def word_items():
    """(word, wanted alignment of its first byte or None) in text order"""
    items = []
    for L in WORD_LENGTHS:
        for a in range(8):
            items.append((_word(L, L + a), a))
    for rep in range(3):
        for w in _twins() + vocab_entry_words() + near_entry_words():
            items.append((w, None))
    for w in vocab_entry_words() + near_entry_words():
        for a in range(8):
            items.append((w, a))
    for k in range(1, 18):
        items.append(("\x00" * k, None))
        items.append(("\x00" * k, (3 * k) % 8))
    for L in (15, 16, 17):                     # words with a leading space: the space is byte 0
        for a in range(8):
            items.append((" " + _word(L - 1, a), a))
    return items


def _place(items) -> str:
    """"\\n" + word per item; digits before the "\\n" move the word's first byte to its alignment"""
    out, n = [], 0
    for w, a in items:
        if a is not None:
            p = (a - (n + 1)) % 8
            out.append("7" * p)
            n += p
        out.append("\n" + w)
        n += 1 + len(w)
    return "".join(out)


@functools.lru_cache(maxsize=None)
def word_loads() -> str:
    return _place(word_items()) + "\n"


@functools.lru_cache(maxsize=None)
def word_load_tails():
    """texts ending in a word of L bytes with d bytes of "\\n" after it, every L of TAIL_LENGTHS
    (1..40, and a 15-byte vocab entry) at every d of TAIL_DISTANCES: 1025 texts; the words before
    shift the alignment"""
    texts = []
    for d in TAIL_DISTANCES:
        for L in TAIL_LENGTHS:
            lead = _place([(_word(3 + (L + d) % 5, d), None), (_word(16, L), (L + d) % 8)])
            texts.append(lead + "\n" + _word(L, L + d) + "\n" * d)
        texts.append("ab\n" + JK15 + "\n" * d)
    return tuple(texts)


def last_word(data: bytes):
    """(start, length, bytes after it) of the last pre-token that is no run of "\\n" """
    toks = [(s, ln) for s, ln in oracle.pretokenize(data) if data[s:s + ln].strip(b"\n")]
    s, ln = toks[-1]
    return s, ln, len(data) - s - ln


# ---------------------------------------------------------------------- uint16 refusals
REFUSAL_REGIONS = ("head", "body_even", "body_odd", "tail", "b", "c_first", "c_later")


@functools.lru_cache(maxsize=None)
def refusal_base() -> str:
    """four chunks without the wide byte: 2048 eight-byte words of 4 ids (the first one of 8 ids,
    so that the next chunk's parts begin at P = 4 mod 8: a head and a tail of 4 uint16 ids); the
    same words, path (a) with T = 4096; eight words of 2048 bytes, path (b); one-byte pre-tokens,
    path (c)"""
    v = [" abababx", " ababxab", " abxabab"]
    words = [v[i % 3] for i in range(2048)]
    chunk_a = "".join(words)
    shift = " xyzxyzx" + "".join(words[1:])
    chunk_b = "".join(xword(2048, 0, i) for i in range(8))
    chunk_c = "".join("0123456789"[(3 * i) % 10] + "xyz"[(7 * i) % 3] for i in range(K_CHUNK // 2))
    return shift + chunk_a + chunk_b + chunk_c


def _refusal_class(region: str) -> str:
    if region.startswith("body"):
        return "body_even" if int(region[4:]) % 2 == 0 else "body_odd"
    if region.startswith("c"):
        return "c_first" if region == "c0" else "c_later"
    return region


@functools.lru_cache(maxsize=None)
def refusal_positions():
    """region -> byte position of an "x" of refusal_base() in chunks 1..3 whose id k_enc_emit<uint16_t>
    stores in that region (Plan.region); "c_later": any round of path (c) after the first"""
    base = refusal_base()
    data = base.encode()
    p = plan_of(base)
    found: dict = {}
    in_a = {"head", "body_even", "body_odd", "tail"}
    for pos in range(K_CHUNK, len(data)):
        if data[pos] != ord("x"):
            continue
        if (pos < 2 * K_CHUNK and in_a <= set(found)) or (2 * K_CHUNK <= pos < 3 * K_CHUNK and "b" in found):
            continue
        found.setdefault(_refusal_class(p.region(p.id_index(data, pos), 2)), pos)
        if len(found) == len(REFUSAL_REGIONS):
            break
    return found


def refusal_text(region: str) -> str:
    base, pos = refusal_base(), refusal_positions()[region]
    assert base[pos] == "x"
    return base[:pos] + WIDE_BYTE + base[pos + 1:]


CASES = {f.__name__: f for f in (path_a_edges, path_b, records_edge, empty_chunks, word_loads)}
