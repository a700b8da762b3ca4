"""CPU checks behind tests/test_gpu_utf8_repair.py: the per-position restatement of the repair rule
equals CPython's decoder, and the case builders build what they claim."""
import pathlib

import utf8_repair_cases as C

MODES = ("replace", "ignore")
UNIT, TILE = 16, 4096   # any geometry will do here: the builders take it as arguments
CORPUS = pathlib.Path(__file__).resolve().parent / "golden" / "fixtures" / "corpus.en"


def _agrees(s):
    for m in MODES:
        assert C.emit(s, m) == C.cpython_repair(s, m), (s.hex(), m)
    assert C.rule_stats(s) == C.cpython_stats(s), s.hex()


def test_rule_equals_cpython_exhaustive():
    assert len(C.BOUNDARY_BYTES) == 27
    n = 0
    for s in C.exhaustive_strings(4):
        _agrees(s)
        n += 1
    assert n == 1 + 27 + 27 ** 2 + 27 ** 3 + 27 ** 4


def test_rule_equals_cpython_random():
    n = 0
    for s in C.random_strings(300_000):
        assert 5 <= len(s) <= 12
        _agrees(s)
        n += 1
    assert n == 300_000


def test_spans_are_first_byte_of_strict_error():
    for s in C.exhaustive_strings(3):
        assert C.cpython_stats(s)[2] == C.strict_position(s)


def test_exhaustive_buffer_is_the_strings_joined():
    buf = C.exhaustive_buffer(2)
    strings = list(C.exhaustive_strings(2))
    for m in MODES:   # the 'A' between two strings ends every unit
        assert C.cpython_repair(buf, m) == b"A".join(C.cpython_repair(s, m) for s in strings)
    assert 2_500_000 < len(C.exhaustive_buffer()) < 3_500_000


def test_seam_cases_put_a_span_on_each_side_of_every_seam():
    seams = C.seam_positions(UNIT, TILE)
    n = 2 * TILE + 37
    assert seams[-1] == n
    before = {s: False for s in seams}
    across = {s: False for s in seams}
    after = {s: False for s in seams}
    names = set()
    for name, buf in C.seam_cases(UNIT, TILE):
        assert len(buf) == n and name not in names
        names.add(name)
        for lo, hi in C.cpython_spans(buf):
            for s in seams:
                if hi <= s and hi > s - 4:
                    before[s] = True
                if lo < s < hi:
                    across[s] = True
                if lo >= s and lo < s + 4:
                    after[s] = True
    assert all(before.values()), before
    assert all(across[s] for s in seams[:-1]), across
    assert all(after[s] for s in seams[:-1]), after   # nothing lies after the end of the text
    assert len(names) == len(C.PATTERNS) * (4 * 9 + 4)   # at the end: offsets -4 .. -1

    buf = C.all_seams_buffer(UNIT, TILE)
    spans = C.cpython_spans(buf)
    for s in seams[:-1]:
        assert any(hi <= s and hi > s - 8 for lo, hi in spans) and any(lo > s and lo < s + 8 for lo, hi in spans)
        assert any(lo < s < hi for lo, hi in spans)


def test_cases_grow_shrink_and_keep():
    ff = b"\xff" * (TILE + 1)
    assert len(C.cpython_repair(ff, "replace")) == 3 * len(ff) and C.cpython_repair(ff, "ignore") == b""
    grown = [len(C.cpython_repair(b, "replace")) > len(b) for _n, b in C.seam_cases(UNIT, TILE)]
    assert any(grown)
    # a 3-byte truncated unit keeps the length and changes the bytes: "clean" is not "same length"
    s = b"ab\xf0\x9f\x98cd"
    assert len(C.cpython_repair(s, "replace")) == len(s) and C.cpython_repair(s, "replace") != s
    mb = C.multibyte_text()
    assert all(b >= 0x80 for b in mb) and C.cpython_stats(mb) == (0, 0, None)
    assert {len(ch.encode()) for ch in mb.decode()} == {2, 3, 4}


def test_dirty_corpus_holds_what_it_claims():
    clean = CORPUS.read_bytes()
    assert C.cpython_stats(clean) == (0, 0, None) and b"\r" not in clean
    d = C.dirty_corpus(clean)
    assert 190 * 1024 < len(d) < 210 * 1024
    spans = C.cpython_spans(d)
    found = {d[lo:hi] for lo, hi in spans}
    for pat in C.BAD_PATTERNS:   # one span per maximal subpart of each pattern
        for lo, hi in C.cpython_spans(b"a" + pat + b"a"):
            assert (b"a" + pat + b"a")[lo:hi] in found
    for pat in C.GOOD_PATTERNS:
        assert pat in d
    assert d.count(b"\r\n") >= 5 and b"\xff\r" in d and b"\xc2\r\n" in d
    assert d.endswith(b"\xf0\x9f\x98") and spans[-1] == (len(d) - 3, len(d))
    w = 65536
    assert any(lo < w < hi for lo, hi in spans) and any(lo < 2 * w < hi for lo, hi in spans)
    for m in MODES:   # the text-mode read is the decode plus universal newlines
        t = C.cpython_read(d, m)
        assert "\r" not in t
        assert t == d.decode("utf-8", m).replace("\r\n", "\n").replace("\r", "\n")
    starts = set()
    for v in C.straddle_variants(d):
        for edge in (w, 2 * w):
            near = [lo - edge for lo, hi in C.cpython_spans(v) if edge - 4 < lo < edge + 4]
            assert near
            starts.update(near)
    assert {-3, -2, -1, 0, 1} <= starts
