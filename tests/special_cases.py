"""Special tokens in Tokenizer.encode: tokenizers and texts on both sides of every threshold at
which csrc/encode.hip treats a special, a match or a segment differently, and the plain-Python
helpers that show (tests/test_special_cases.py, on the CPU) that a case reaches what it claims.

The library's special list is deduplicated, longest first by UTF-8 length, equal lengths in
first-occurrence order (library_order).  k_find_specials records every (position, special) at
which a special's bytes stand, overlaps included (raw_matches restates that list); the matches
become the segment table on the device when no two of them overlap, and go through the host's
leftmost-longest loop otherwise (segments restates the result); k_enc_scan4 keeps the segments
of a chunk's window in LDS when there are at most kSegLds of them (window_segment_counts).

Every case uses the 256 bytes, the merges of MERGES (multi-id and one-id words both occur) and
every special as a vocab entry of its own; "missing" is the one case whose specials are absent
from the vocab, with pairwise different lengths (the reference gives equal-length missing
specials ids in set order, and the two references disagree there: that ambiguity is kept out).
A text interleaves its specials' occurrences and near-misses ("<|", "|>", a special without its
last character, a special with another last byte) with pre-tokens of every class (FILL).

Families (CASES; a case's `texts` are each encoded on their own):
  lengths_ascii, lengths_utf8   specials of LENGTHS bytes, from 17 up with a twin differing at
                    byte 16 and a twin differing in the last byte; at most kSpLds per case, so
                    every one is matched under the LDS masks; the utf8 ones start with bytes
                    >= 0xC0 (first-byte bitmap words 6 and 7)
  many              140 specials: the long ones at index < kSpLds, the short ones beyond
  dense_single      a one-byte special, > kSpBuf matches in a 4 KiB stretch, no overlaps
  dense_prefix      "<|" and "<" at the same positions: as dense, on the host path
  overlap           aa, aba, ab/bc, "a b"/"b c", < <|a <|a| <|a|>, <|endoftext|> and its double
  overlap_twin      the same text with specials whose raw matches never overlap
  context_each      BEFORE x AFTER around a special, every combination a text of its own
  context_joined    the same combinations joined by a letter word
  placement         a 13-byte and a 200-byte special at offsets 0, 1, 62, 63, 64 of a 64-byte
                    block, 1, 7, 13 bytes before a 16 KiB boundary, on it, ending on it, and
                    beginning in the last 16 bytes of a chunk's halo
  seg_few, seg_many at most kSegLds segments in every chunk window / far more in one
  seg_64, seg_65    equal but for one special: the second chunk's window holds 64 / 65
  missing           three specials that are not in the vocab, of different lengths
"""
from __future__ import annotations

import bisect
import functools
import random

# thresholds, as the source has them
K_SP_LDS = 64        # kSpLds    csrc/encode.hip:113
K_SP_BUF = 2048      # kSpBuf    csrc/encode.hip:114
K_SEG_LDS = 64       # kSegLds   csrc/encode.hip:402
K_CHUNK = 16384      # kChunk    csrc/stage.h:26
K_HALO = 1024        # kHalo     csrc/stage.h:27
K_WIN = K_CHUNK + K_HALO   # kWin  csrc/stage.h:28
K_PRE = 16           # kPre      csrc/stage2.h:41
K_POST = 16          # kPost     csrc/stage2.h:42
STRETCH = 256 * 16   # bytes a workgroup of k_find_specials sees of a small text: 256 threads, one
                     # 16-byte unit each (csrc/encode.hip:214-215, the grid of :1830)
BLOCK = 64           # bytes per thread of k_enc_scan4 (csrc/encode.hip:672)


def match_capacity(n: int) -> int:
    """the first size of the global match list (csrc/encode.hip:1824)"""
    return max(1024, n // 64)


EOT = "<|endoftext|>"
SP200 = "<|" + "long special token " * 10 + "is 200|>"
assert len(EOT) == 13 and len(SP200.encode()) == 200

# (a, b) as strings; each product becomes a vocab entry.  " the", "'s", "'ll", "é", "  ", "\n\n",
# "12" and "abc" are one id; " cat", "xyz", " naïve", "東京" and most others several.
_STR_MERGES = [(" ", "t"), ("h", "e"), (" t", "he"), ("t", "he"), ("'", "s"), ("l", "l"), ("'", "ll")]
_BYTE_MERGES = [(b"\xc3", b"\xa9"), (b" ", b" "), (b"\n", b"\n"), (b"1", b"2"), (b"a", b"b"), (b"ab", b"c"),
                (b"a", b"t"), (b" ", b"c"), (b"x", b"y"), (b"!", b"!"), (b"b", b"c"), (b" ", b"a"),
                (b"a", b"a"), (b"aa", b"aa"), (b"\xe6\x9d", b"\xb1"), (b"o", b"n"), (b"e", b"n"), (b"<", b"|"),
                (b"|", b">"), (b"en", b"d"), (b"t", b"e"), (b"te", b"x"), (b"tex", b"t"), (b"o", b"f"),
                (b"\xc2", b"\xa0"), (b"3", b"4"), (b"a", b" "), (b" ", b"b")]
MERGES = [(a.encode(), b.encode()) for a, b in _STR_MERGES] + _BYTE_MERGES

# pre-tokens of every class: letter, 2- and 3-byte letter, digit, punctuation, contraction, one
# space, space runs, \n, \t, U+00A0, U+3000
FILL = ["the", " the", " cat", "abc", " xyz", "é", " naïve", "東京", " 東", "ß", "12", " 1234", "7", "!!", ",", " ?",
        "'s", "'ll", " ", "  ", "   ", "\n", "\n\n", "\t", "\u00a0", "\u3000", " \n", "at", "aa", "b"]
NEAR = ["<|", "|>", "<", "|"]


class Case:
    def __init__(self, name, family, specials, texts, in_vocab=True, **claims):
        self.name, self.family = name, family
        self.specials = list(specials)
        self.texts = tuple(texts)
        self.text = self.texts[0]            # the main text (the only one, for most cases)
        self.claims = claims
        self.vocab = {i: bytes([i]) for i in range(256)}
        self.merges = list(MERGES)
        for a, b in self.merges:
            self.vocab[len(self.vocab)] = a + b
        if in_vocab:
            have = set(self.vocab.values())
            for s in self.specials:
                if s.encode("utf-8") not in have:
                    have.add(s.encode("utf-8"))
                    self.vocab[len(self.vocab)] = s.encode("utf-8")


# ---------------------------------------------------------------------- helpers, plain Python
def library_order(specials):
    """the library's list: first occurrences, longest first by UTF-8 length, stable -- after
    bpe_amd.Tokenizer's own stable sort by character length (csrc/encode.hip:1716-1721)"""
    seen = list(dict.fromkeys(specials))
    seen.sort(key=len, reverse=True)
    seen.sort(key=lambda s: len(s.encode("utf-8")), reverse=True)
    return seen


def raw_matches(data: bytes, specials):
    """every (byte position, index in library_order(specials)) at which that special's bytes
    stand in data, overlaps included, sorted: what k_find_specials lists"""
    out = []
    for k, s in enumerate(library_order(specials)):
        b = s.encode("utf-8")
        p = data.find(b)
        while p >= 0:
            out.append((p, k))
            p = data.find(b, p + 1)
    out.sort()
    return out


def special_lengths(specials):
    return [len(s.encode("utf-8")) for s in library_order(specials)]


def has_overlap(matches, lens) -> bool:
    """two raw matches share a byte (two at one position included)"""
    end = 0
    for p, k in matches:
        if p < end:
            return True
        end = max(end, p + lens[k])
    return False


def stretch_counts(matches, lead: int = 0) -> dict:
    """raw matches per 4 KiB stretch of a text whose first byte lies `lead` bytes past a 16-byte
    boundary"""
    out: dict = {}
    for p, _k in matches:
        out[(p + lead) // STRETCH] = out.get((p + lead) // STRETCH, 0) + 1
    return out


def segments(n: int, matches, lens):
    """[(start, end, special index or -1)]: re.split's leftmost matches, the longest special at
    a position first; no empty normal segment"""
    segs, cur = [], 0
    for p, k in matches:
        if p < cur:
            continue
        if p > cur:
            segs.append((cur, p, -1))
        segs.append((p, p + lens[k], k))
        cur = p + lens[k]
    if cur < n:
        segs.append((cur, n, -1))
    return segs


def window_segment_counts(n: int, segs):
    """per 16 KiB chunk, the segments k_enc_scan4 sees for it: from the one holding base - kPre,
    those with start below base + kWin + kPost (csrc/encode.hip:635-645)"""
    starts = [s for s, _e, _k in segs]
    out = []
    for base in range(0, n, K_CHUNK):
        w0, w1 = max(base - K_PRE, 0), base + K_WIN + K_POST
        k0 = max(bisect.bisect_right(starts, w0) - 1, 0)
        out.append(bisect.bisect_left(starts, w1) - k0)
    return out


def case_matches(case: Case, text=None):
    data = (case.text if text is None else text).encode("utf-8")
    return data, raw_matches(data, case.specials), special_lengths(case.specials)


def cut_documents(text: str, n_docs: int, seed: int):
    """the text cut into n_docs documents at arbitrary characters, inside specials included"""
    r = random.Random(seed)
    cuts = sorted(r.sample(range(1, len(text)), n_docs - 1))
    return [text[a:b] for a, b in zip([0] + cuts, cuts + [len(text)])]


def last_changed(s: str) -> str:
    """s with another last byte (the last character's lowest bit flipped)"""
    return s[:-1] + chr(ord(s[-1]) ^ 1)


def near_misses(specials):
    return NEAR + [s[:-1] for s in specials if len(s) > 1] + [last_changed(s) for s in specials]


def mix(seed: int, specials, n_items: int, p_special=0.3, p_near=0.1, extra=()):
    """n_items drawn from the specials, their near-misses, `extra` and FILL"""
    r = random.Random(seed)
    near = near_misses(specials) + list(extra)
    parts = []
    for _ in range(n_items):
        x = r.random()
        if x < p_special:
            parts.append(r.choice(specials))
        elif x < p_special + p_near:
            parts.append(r.choice(near))
        else:
            parts.append(r.choice(FILL))
    return "".join(parts)


def cover(seed: int, specials) -> str:
    """every special, every special without its last character and every special with another
    last byte, once each, between FILL words"""
    r = random.Random(seed)
    parts = []
    for sp in specials:
        parts += [r.choice(FILL), sp, r.choice(FILL), sp[:-1], r.choice(FILL), last_changed(sp), r.choice(FILL)]
    return "".join(parts)


def safe_split(data: bytes, pos: int) -> int:
    """bpe_safe_split (csrc/api.hip:545): the largest p <= pos with a U+0020 at p between two
    ASCII non-space bytes, or 0"""
    def ok(b):
        return b < 0x80 and b != 0x20 and not 0x09 <= b <= 0x0D
    n = len(data)
    if n < 3:
        return 0
    for p in range(min(pos, n - 2), 0, -1):
        if data[p] == 0x20 and ok(data[p - 1]) and ok(data[p + 1]):
            return p
    return 0


def spanned_first_cuts(data: bytes, matches, lens, ranks: int) -> int:
    """of the slab boundaries n / ranks * r, how many have their first safe split point strictly
    inside a raw match: encode over `ranks` devices has to look further back there
    (encode_cuts, csrc/encode.hip:2206)"""
    count = 0
    for r in range(1, ranks):
        p = safe_split(data, len(data) // ranks * r)
        count += any(q < p < q + lens[k] for q, k in matches)
    return count


_PAD = " the cat's 12 dogs!!  ran\nat 7,\tabc xyz 'll  go "


def pad(k: int, phase: int = 0) -> str:
    """k ASCII bytes of mixed pre-tokens (no '<')"""
    s = _PAD[phase % len(_PAD):] + _PAD * (k // len(_PAD) + 1)
    return s[:k]


# ---------------------------------------------------------------------- lengths
LENGTHS = (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 200, 1100)
TWIN_FROM = 17


def _ascii_special(L: int, tag: str) -> str:
    body = (f"<{tag}{L}:" + "abcdefghijklmnopqrstuvwxyz0123456789" * 40)
    return {1: "^", 2: "~" + tag[0]}.get(L) or body[:L - 1] + ">"


_MARK2, _MARK3 = "àáâãäåæçèêëìíîïð", "一二三四五六七八九十"


def _utf8_special(L: int) -> str:
    """L bytes of 2- and 3-byte characters.  The first character is one that no other length
    uses and that stands nowhere else, so no special is part of another."""
    n3 = L // 3
    while (L - 3 * n3) % 2:
        n3 -= 1
    n2 = (L - 3 * n3) // 2
    c3, c2 = "東京都語文字", "éñüßøö"
    i = LENGTHS.index(L)
    s = "".join(c2[(j + i) % 6] for j in range(n2)) + "".join(c3[(j + i) % 6] for j in range(n3))
    s = (_MARK2[i] if n2 else _MARK3[i % 10]) + s[1:]
    assert len(s.encode("utf-8")) == L
    return s


def _with_twins(make):
    """(specials, {length: [special, twin differing in the character that holds byte 16, twin
    differing in the last character]}); a twin differs in the last byte of that character only,
    and at 17 bytes the two twins are one"""
    out, by_len = [], {}
    for L in LENGTHS:
        s = make(L)
        if s is None:
            continue
        group = [s]
        if L >= TWIN_FROM:
            ends = []                          # byte offset past each character
            for c in s:
                ends.append((ends[-1] if ends else 0) + len(c.encode("utf-8")))
            for pos in (next(i for i, e in enumerate(ends) if e > 16), len(s) - 1):
                t = s[:pos] + chr(ord(s[pos]) ^ 1) + s[pos + 1:]
                assert t.encode("utf-8")[:16] == s.encode("utf-8")[:16] and len(t.encode("utf-8")) == L
                if t not in group:
                    group.append(t)
        out += group
        by_len[L] = group
    assert len(set(out)) == len(out)
    return out, by_len


def _lengths_case(name, make, seed):
    specials, by_len = _with_twins(make)
    r = random.Random(seed)
    parts = []
    for rep in range(3):                       # every special three times, then the mix
        order = list(specials)
        r.shuffle(order)
        for s in order:
            parts += [r.choice(FILL), s, r.choice(FILL), s[:-1], r.choice(FILL), last_changed(s), r.choice(FILL)]
    text = "".join(parts) + mix(seed + 1, [s for s in specials if len(s.encode()) < 200], 1500)
    return Case(name, "lengths", specials, [text], by_len=by_len)


@functools.lru_cache(maxsize=None)
def lengths_ascii():
    return _lengths_case("lengths_ascii", lambda L: _ascii_special(L, "A"), 101)


@functools.lru_cache(maxsize=None)
def lengths_utf8():
    return _lengths_case("lengths_utf8", lambda L: None if L == 1 else _utf8_special(L), 102)


# ---------------------------------------------------------------------- many
@functools.lru_cache(maxsize=None)
def many():
    longs = [f"<|long{i:03d}|>" for i in range(70)]
    shorts = ([f"@{c}" for c in "abcdefghijklmnopqrstuvwxyz"] + [f"%{c}" for c in "ABCDEFGHIJKLMNOPQRSTUVWXYZ"]
              + [f"#{d}" for d in "0123456789"] + ["€", "¤", "§x", "~", "^", "`", "&&", "$$"])
    specials = []
    for i in range(max(len(longs), len(shorts))):      # given interleaved: the library sorts them
        specials += longs[i:i + 1] + shorts[i:i + 1]
    text = cover(200, specials) + mix(201, specials, 6000, extra=["@", "%", "#", "<|long", "<|long07", "|>"])
    return Case("many", "many", specials, [text])


# ---------------------------------------------------------------------- dense
def _dense_text(unit: str, seed: int) -> str:
    """90 KB: three runs of 3 x 4 KiB of `unit` and a little else, between ordinary text"""
    r = random.Random(seed)
    parts = [mix(seed, [unit], 2500, p_special=0.02)]
    for _ in range(3):
        run, size = [], 0
        while size < 3 * STRETCH:
            x = unit * r.randrange(1, 12) + r.choice(["", "", "a", " ", "7", "é", "\n", " b"])
            run.append(x)
            size += len(x.encode("utf-8"))
        parts += ["".join(run), mix(seed + 7, [unit], 5000, p_special=0.02)]
    return "".join(parts)


@functools.lru_cache(maxsize=None)
def dense_single():
    return Case("dense_single", "dense", ["|"], [_dense_text("|", 301)], overlaps=False)


@functools.lru_cache(maxsize=None)
def dense_prefix():
    return Case("dense_prefix", "dense", ["<", "<|"], [_dense_text("<|", 302)], overlaps=True)


# ---------------------------------------------------------------------- overlap
OVERLAP_SPECIALS = ["aa", "aba", "ab", "bc", "a b", "b c", "<", "<|a", "<|a|", "<|a|>", EOT, EOT + EOT]
OVERLAP_TWIN_SPECIALS = [EOT, "<|a|>", "bc"]
A_RUNS = ["a" * k for k in range(1, 10)]
OVERLAP_ITEMS = A_RUNS + ["aba", "ababa", "abab", "abababa", "abc", "abcbc", "aabc", "a b", "b c", "a b c", "a b c b c",
                          "xa b cx", "a  b", "<", "<|", "<|a", "<|a|", "<|a|>", "<|a|>>", "<<|a|>", "<|a|a|>", "<|a<|a|>",
                          EOT, EOT * 2, EOT * 3, EOT + EOT[:-1], EOT[:-1] + EOT, "<" + EOT]


@functools.lru_cache(maxsize=None)
def _overlap_text():
    r = random.Random(401)
    seps = [" ", "\n", "!", "7", " x", "é", "  ", "'s", " the ", "\t", "東", ". "]
    parts = []
    for rep in range(60):
        order = list(OVERLAP_ITEMS)
        r.shuffle(order)
        for it in order:
            parts += [it, r.choice(seps)]
        parts.append(mix(402 + rep, ["a b c", "b c a b"], 12, p_special=0.5))
    return "".join(parts)


@functools.lru_cache(maxsize=None)
def overlap():
    return Case("overlap", "overlap", OVERLAP_SPECIALS, [_overlap_text()], overlaps=True)


@functools.lru_cache(maxsize=None)
def overlap_twin():
    return Case("overlap_twin", "overlap", OVERLAP_TWIN_SPECIALS, [_overlap_text()], overlaps=False)


# ---------------------------------------------------------------------- context
CTX, CTX_OTHER = "<|sp|>", "<|other|>"
BEFORE = {"start": "", "letter": "a", "letter3": "東", "digit": "7", "punct": "!", "apos": "a'", "space1": "a ",
          "space2": "a  ", "newline": "a\n", "tab": "a\t", "nbsp": "a\u00a0"}
AFTER = {"end": "", "letter": "b", "space_letter": " b", "space2_letter": "  b", "apos_s": "'s", "digit": "5",
         "newline": "\n", "same": CTX, "other": CTX_OTHER}
JOINER = "zq"


def _before_class(text: str, p: int) -> str:
    if p == 0:
        return "start"
    c = text[p - 1]
    if c == " ":
        return "space2" if p >= 2 and text[p - 2] == " " else "space1"
    named = {"\n": "newline", "\t": "tab", "\u00a0": "nbsp", "'": "apos"}
    if c in named:
        return named[c]
    if c.isdigit():
        return "digit"
    if c.isalpha():
        return "letter3" if len(c.encode("utf-8")) == 3 else "letter"
    return "punct"


def _after_class(text: str, p: int) -> str:
    rest = text[p:]
    if not rest:
        return "end"
    for name, lead in (("same", CTX), ("other", CTX_OTHER), ("apos_s", "'s"), ("newline", "\n")):
        if rest.startswith(lead):
            return name
    if rest[0].isdigit():
        return "digit"
    if rest[0].isalpha():
        return "letter"
    if rest.startswith("  ") and rest[2:3].isalpha():
        return "space2_letter"
    if rest.startswith(" ") and rest[1:2].isalpha():
        return "space_letter"
    return "?"


def context_pairs(texts):
    """{(before class, after class)} over the occurrences of CTX in the texts"""
    out = set()
    for t in texts:
        p = t.find(CTX)
        while p >= 0:
            out.add((_before_class(t, p), _after_class(t, p + len(CTX))))
            p = t.find(CTX, p + 1)
    return out


def _context_texts():
    return [b + CTX + a for b in BEFORE.values() for a in AFTER.values()]


@functools.lru_cache(maxsize=None)
def context_each():
    return Case("context_each", "context", [CTX, CTX_OTHER], _context_texts())


@functools.lru_cache(maxsize=None)
def context_joined():
    return Case("context_joined", "context", [CTX, CTX_OTHER], [JOINER.join(_context_texts())])


# ---------------------------------------------------------------------- placement
BLOCK_OFFSETS = (0, 1, 62, 63, 64)
BEFORE_BOUNDARY = (1, 7, 13, 0)             # the special starts this many bytes before a 16 KiB boundary


@functools.lru_cache(maxsize=None)
def placement():
    """-> the case; claims["at"] = [(what, special, byte position)]"""
    at = []
    k = 2
    for sp, step in ((EOT, 2), (SP200, 6)):
        for o in BLOCK_OFFSETS:
            at.append((f"block+{o}", sp, BLOCK * k + o))
            k += step
    b = 1
    for sp in (EOT, SP200):
        for d in BEFORE_BOUNDARY:
            at.append((f"boundary-{d}", sp, b * K_CHUNK - d))
            b += 1
        at.append(("ends-on-boundary", sp, b * K_CHUNK - len(sp)))
        b += 1
    for sp, back in ((EOT, 11), (SP200, 16)):   # in the last 16 bytes of chunk b - 1's halo
        at.append(("halo-end", sp, b * K_CHUNK + K_HALO - back))
        b += 1
    parts, size = [], 0
    for _what, sp, p in at:
        assert p >= size, (p, size)
        parts += [pad(p - size, size), sp]
        size = p + len(sp)
    parts.append(pad(300, size))
    return Case("placement", "placement", [EOT, SP200], ["".join(parts)], at=at)


# ---------------------------------------------------------------------- segments per chunk
def _spaced(n_bytes: int, every: int, specials, seed: int) -> str:
    r = random.Random(seed)
    parts, size = [], 0
    while size < n_bytes:
        k = every + r.randrange(0, max(every // 4, 1))
        sp = r.choice(specials)
        parts += [pad(k, size), sp]
        size += k + len(sp)
    return "".join(parts) + pad(50)


@functools.lru_cache(maxsize=None)
def seg_few():
    return Case("seg_few", "segments", [EOT, "<|pad|>"], [_spaced(3 * K_CHUNK, 900, [EOT, "<|pad|>"], 601)])


@functools.lru_cache(maxsize=None)
def seg_many():
    text = _spaced(K_CHUNK + 300, 900, [EOT], 602) + _spaced(K_CHUNK, 9, [EOT, "<|pad|>"], 603) + pad(K_CHUNK)
    return Case("seg_many", "segments", [EOT, "<|pad|>"], [text])


def _seg_pair(third: bool):
    """Three chunks; in the second chunk's window [kChunk - kPre, kChunk + kWin + kPost): the
    normal segment holding its first byte, 30 lone specials (two segments each) and one run of
    two specials (three segments with the text behind it): 64.  A third special in that run,
    where the other text has 13 letters: 65."""
    parts = [pad(K_CHUNK + 100)]
    size = K_CHUNK + 100
    for _ in range(30):
        parts += [EOT, pad(487, size)]
        size += 500
    parts += [EOT, EOT, EOT if third else "thirteenchars", pad(K_CHUNK * 3 - 200 - size - 39, size)]
    return "".join(parts) + pad(200)


@functools.lru_cache(maxsize=None)
def seg_64():
    return Case("seg_64", "segments", [EOT], [_seg_pair(False)], window1=64)


@functools.lru_cache(maxsize=None)
def seg_65():
    return Case("seg_65", "segments", [EOT], [_seg_pair(True)], window1=65)


# ---------------------------------------------------------------------- missing from the vocab
@functools.lru_cache(maxsize=None)
def missing():
    specials = ["<|m1|>", "<|miss2|>", "<|missing3|>"]
    assert len({len(s) for s in specials}) == len(specials)
    return Case("missing", "missing", specials, [cover(700, specials) + mix(701, specials, 3000)], in_vocab=False)


CASES = {f.__name__: f for f in (lengths_ascii, lengths_utf8, many, dense_single, dense_prefix, overlap, overlap_twin,
                                 context_each, context_joined, placement, seg_few, seg_many, seg_64, seg_65, missing)}


# ---------------------------------------------------------------------- training: the special filter
# k_collect_words (csrc/train_setup.h) and k_list_table (csrc/accum.hip) drop the unique words equal
# to a special, read through one of three key forms: up to 7 bytes, 8..16 bytes, longer.
TRAIN_VOCAB = 400
WORD_LENGTHS = (2, 7, 8, 16, 17, 40)
WORDS = {L: " " + ("qjzkvx"[i] * 40)[:L - 2] + "m" if L > 2 else " q" for i, L in enumerate(WORD_LENGTHS)}
assert all(len(w) == L for L, w in WORDS.items())
OTHER_WORDS = ["é", "\n\n", "'s"]
SIXTY = [" w" + chr(97 + i // 8) + chr(97 + i % 8) for i in range(60)]


@functools.lru_cache(maxsize=None)
def train_corpus() -> str:
    """about 200 KB in which the special lists' words are frequent pre-tokens"""
    r = random.Random(801)
    common = [" the", " the", " cat", " then", " that", " hat", " 12", ",", " other"]
    parts = []
    for _ in range(27000):
        x = r.random()
        if x < 0.30:
            parts.append(WORDS[r.choice(WORD_LENGTHS)])
        elif x < 0.36:
            parts.append("7é")
        elif x < 0.42:
            parts.append(r.choice(common).strip() + "'s")
        elif x < 0.47:
            parts.append("\n\n the")
        elif x < 0.62:
            parts.append(SIXTY[int(60 * r.random() ** 1.5)])
        elif x < 0.64:
            parts.append(EOT)
        else:
            parts.append(r.choice(common))
    return "".join(parts)


# name -> (special list, whether the words it drops change which merges are chosen)
TRAIN_LISTS = {
    "none": ([], False),
    "words": ([WORDS[L] for L in WORD_LENGTHS] + OTHER_WORDS, True),
    "inline_only": ([WORDS[2], WORDS[7]], True),
    "mid_only": ([WORDS[8], WORDS[16]], True),
    "long_only": ([WORDS[17], WORDS[40]], True),
    "others_only": (OTHER_WORDS, True),
    "one_byte": (["q", "\n", "e"], False),                  # dedupe against the byte entries: no slot taken
    "duplicates": (["é", WORDS[7], "é", EOT, WORDS[7], WORDS[17], EOT], True),
    "never": ([" neveroccurs", "zzzzzzzzzzzzzzzzzzzzzzzz", " qqqqqm"], False),
    "no_pretoken": ([EOT, "the cat", "<|end"], False),          # never a single pre-token
    "merge_products": (["th", "he", " t", "xx", "xxxx"], False),          # Vocab.add_token adds nothing for those merges
    "seventy": ([WORDS[L] for L in WORD_LENGTHS] + OTHER_WORDS + [EOT] + SIXTY, True),
}
assert len(set(TRAIN_LISTS["seventy"][0])) == 70
