"""The UTF-8 repair's rule restated per position, the CPython oracles, and the case builders of
tests/test_gpu_utf8_repair.py (their claims are asserted in tests/test_utf8_repair_cases.py).

errors="replace" / "ignore" are CPython's: each maximal subpart of an ill-formed subsequence is
one U+FFFD, or nothing.  The kernel decides every position from s[i - 3 .. i + 3] and the end of
the text; emit() below is that decision written down, byte for byte, without a decoder."""
import codecs
import io
import itertools
import random

# the bytes at which the lead-byte table changes, plus ASCII, CR and LF
BOUNDARY_BYTES = bytes.fromhex("41200D0A7F808F909FA0BFC0C1C2DFE0E1ECEDEEEFF0F1F3F4F5FF")
FFFD = b"\xef\xbf\xbd"

# ill-formed patterns (each maximal subpart is one span) and well-formed ones
BAD_PATTERNS = [bytes.fromhex(h) for h in ("E080", "EDA080", "F09080", "F490", "C2", "80808080", "FF")]
GOOD_PATTERNS = [bytes.fromhex(h) for h in ("C3A9", "E282AC", "F09F9880")]
TRUNCATED_THEN_LEAD = bytes.fromhex("F09F98C3A9")   # F0 9F 98 followed by a lead (of a well-formed C3 A9)
PATTERNS = BAD_PATTERNS + GOOD_PATTERNS + [TRUNCATED_THEN_LEAD]


def _is_cont(b):
    return (b & 0xC0) == 0x80


def _lead(b0):
    """(needed length, lowest and highest second byte); needed 0: never a lead."""
    if b0 < 0x80:
        return 1, 0x80, 0xBF
    if 0xC2 <= b0 <= 0xDF:
        return 2, 0x80, 0xBF
    if b0 == 0xE0:
        return 3, 0xA0, 0xBF
    if 0xE1 <= b0 <= 0xEC or 0xEE <= b0 <= 0xEF:
        return 3, 0x80, 0xBF
    if b0 == 0xED:
        return 3, 0x80, 0x9F
    if b0 == 0xF0:
        return 4, 0x90, 0xBF
    if 0xF1 <= b0 <= 0xF3:
        return 4, 0x80, 0xBF
    if b0 == 0xF4:
        return 4, 0x80, 0x8F
    return 0, 0x80, 0xBF


def _unit(s, q):
    """The unit that starts at the non-continuation byte s[q]: (length, complete)."""
    need, lo, hi = _lead(s[q])
    length = 1
    if need >= 2 and q + 1 < len(s) and lo <= s[q + 1] <= hi:
        length = 2
        if need >= 3 and q + 2 < len(s) and _is_cont(s[q + 2]):
            length = 3
            if need == 4 and q + 3 < len(s) and _is_cont(s[q + 3]):
                length = 4
    return length, length == need


def classify(s, i):
    """'ok' (the byte is copied), 'start' (first byte of an ill-formed unit) or 'rest' (another
    byte of one), from s[i - 3 .. i + 3] and len(s) alone."""
    b = s[i]
    if b < 0x80:
        return "ok"
    if not _is_cont(b):
        return "ok" if _unit(s, i)[1] else "start"
    for d in (1, 2, 3):
        q = i - d
        if q < 0:
            break
        if not _is_cont(s[q]):
            length, complete = _unit(s, q)
            if d < length:
                return "ok" if complete else "rest"
            return "start"   # a stray: the unit before it ends earlier
    return "start"


def emit(s, mode):
    """The repaired bytes by the per-position rule."""
    out = bytearray()
    for i in range(len(s)):
        c = classify(s, i)
        if c == "ok":
            out.append(s[i])
        elif c == "start" and mode == "replace":
            out += FFFD
    return bytes(out)


def rule_stats(s):
    """(n_units, n_bytes, first or None) by the per-position rule."""
    cls = [classify(s, i) for i in range(len(s))]
    starts = [i for i, c in enumerate(cls) if c == "start"]
    return len(starts), sum(c != "ok" for c in cls), (starts[0] if starts else None)


# ------------------------------------------------------------------ CPython, the oracle
def cpython_repair(raw, mode):
    return raw.decode("utf-8", mode).encode("utf-8")


def cpython_read(raw, mode):
    """The text a file opened with open(path, encoding="utf-8", errors=mode) reads."""
    return io.TextIOWrapper(io.BytesIO(raw), encoding="utf-8", errors=mode, newline=None).read()


_spans = []


def _counting_handler(err):
    _spans.append((err.start, err.end))
    return ("", err.end)


codecs.register_error("bpe355-count-spans", _counting_handler)


def cpython_spans(raw):
    """The (start, end) of every span CPython's decoder hands to an error handler."""
    _spans.clear()
    raw.decode("utf-8", "bpe355-count-spans")
    return list(_spans)


def cpython_stats(raw):
    """(n_units, n_bytes, first or None) from the counting handler."""
    sp = cpython_spans(raw)
    return len(sp), sum(e - s for s, e in sp), (sp[0][0] if sp else None)


def strict_position(raw):
    try:
        raw.decode("utf-8")
    except UnicodeDecodeError as e:
        return e.start
    return None


# ------------------------------------------------------------------ case sets
def exhaustive_strings(max_len=4):
    for n in range(max_len + 1):
        for t in itertools.product(BOUNDARY_BYTES, repeat=n):
            yield bytes(t)


def exhaustive_buffer(max_len=4):
    """Every string of length <= max_len over BOUNDARY_BYTES, an ASCII 'A' between them: the 'A'
    ends every unit, so the buffer's repair is the strings' repairs joined the same way."""
    return b"A".join(exhaustive_strings(max_len))


def random_strings(count, seed=355):
    rnd = random.Random(seed)
    for _ in range(count):
        yield bytes(rnd.choice(BOUNDARY_BYTES) for _ in range(rnd.randint(5, 12)))


def seam_positions(unit, tile):
    """Where the kernel's paths meet in a buffer of 2 * tile + 37 bytes: a vector's end, a wave's
    end, a tile's end, the second tile's end (the start of the ragged last tile), the text's end."""
    return [unit, 64 * unit, tile, 2 * tile, 2 * tile + 37]


def seam_cases(unit, tile):
    """(name, bytes): each pattern at every offset from -4 to +4 around every seam of an ASCII
    buffer of 2 * tile + 37 bytes (a pattern that would pass the end is cut there: a truncated
    tail)."""
    n = 2 * tile + 37
    base = bytes(0x61 + i % 26 for i in range(n))
    for pat in PATTERNS:
        for seam in seam_positions(unit, tile):
            for d in range(-4, 5):
                at = seam + d
                if at < 0 or at >= n:
                    continue
                buf = bytearray(base)
                cut = pat[:n - at]
                buf[at:at + len(cut)] = cut
                yield f"{pat.hex()}@{seam}{d:+d}", bytes(buf)


def all_seams_buffer(unit, tile):
    """One buffer with an ill-formed span on each side of every seam (for the stats and the
    pointer-offset cases)."""
    n = 2 * tile + 37
    buf = bytearray(0x61 + i % 26 for i in range(n))
    for k, seam in enumerate(seam_positions(unit, tile)):
        pat = BAD_PATTERNS[k % len(BAD_PATTERNS)]
        lo = seam - len(pat) - 1
        buf[lo:lo + len(pat)] = pat                      # ends before the seam
        if seam + 1 + len(pat) <= n:
            buf[seam + 1:seam + 1 + len(pat)] = pat      # starts after it
        buf[seam - 1:seam + 1] = b"\xe2\x82"[:n - (seam - 1)]   # and a truncated E2 82 across it
    return bytes(buf)


def multibyte_text(n_chars=3000):
    """Well-formed text without a single ASCII byte."""
    alphabet = "éßπЖ中文€😀𐍈"
    return "".join(alphabet[i % len(alphabet)] for i in range(n_chars)).encode("utf-8")


def dirty_corpus(clean, target=200 * 1024, window=65536):
    """About `target` bytes of `clean` (well-formed UTF-8 text) with ill-formed spans inserted:
    one of each pattern, some \\r\\n, a span directly before a \\r, spans that straddle the raw
    offsets window and 2 * window, and a truncated sequence as the very last bytes.  The
    insertions overwrite ASCII letters and spaces only."""
    src = clean
    while len(src) < target:
        src += clean
    buf = bytearray(src[:target])
    # end on a character, not inside one
    while buf and _is_cont(buf[-1]):
        buf.pop()
    if buf and buf[-1] >= 0xC0:
        buf.pop()

    def ascii_run(at, length):
        """the first position >= at from which `length` ASCII letters or spaces run"""
        i = at
        while True:
            if all(b == 0x20 or 0x61 <= b <= 0x7A for b in buf[i:i + length]) and len(buf[i:i + length]) == length:
                return i
            i += 1

    at = 1000
    for pat in PATTERNS:
        i = ascii_run(at, len(pat) + 2)
        buf[i + 1:i + 1 + len(pat)] = pat
        at = i + 3000
    for k in range(5):   # \r\n line ends
        i = ascii_run(at, 4)
        buf[i + 1:i + 3] = b"\r\n"
        at = i + 2500
    i = ascii_run(at, 6)   # a span directly before a \r, then one before \r\n
    buf[i + 1:i + 3] = b"\xff\r"
    i = ascii_run(i + 100, 6)
    buf[i + 1:i + 4] = b"\xc2\r\n"
    # straddling the raw window edges: a truncated F0 9F 98 from 2 before the first, a truncated
    # E2 82 from 1 before the second (straddle_variants lays out every offset -3 .. +1)
    for lo, pat in ((window - 2, b"\xf0\x9f\x98\x41"), (2 * window - 1, b"\xe2\x82")):
        buf[lo - 4:lo + len(pat) + 4] = b"x" * (len(pat) + 8)
        buf[lo:lo + len(pat)] = pat
    return bytes(buf) + b" end\xf0\x9f\x98"   # a truncated sequence as the very last bytes


def straddle_variants(dirty, window=65536):
    """dirty with one more span laid over each of the raw offsets window and 2 * window, starting
    at offset -3 .. +1 from the edge: five corpora."""
    out = []
    pats = (b"\xf0\x9f\x98", b"\xf0\x9f\x98\x41", b"\xe2\x82", b"\xed\xa0\x80", b"\x80\x80")
    for d, pat in zip(range(-3, 2), pats):
        buf = bytearray(dirty)
        for edge in (window, 2 * window):
            lo = edge + d
            # keep the neighbourhood plain ASCII so that the span is exactly the pattern's
            buf[lo - 4:lo + len(pat) + 4] = b"x" * (len(pat) + 8)
            buf[lo:lo + len(pat)] = pat
        out.append(bytes(buf))
    return out
