"""CPU: the inputs of tests/emit_cases.py reach what they claim, by the oracle alone.

The restated constants equal the constexpr lines of csrc/stage.h and csrc/encode.hip and the
emit's branch conditions stand in the source as the plan restates them, so a retune fails here
and not in the premise of tests/test_gpu_emit.py.  Then, per case, the parts plan() finds: every
assertion names the class it looks for.
"""
from __future__ import annotations

import functools
import pathlib
import re

import numpy as np
import pytest

import emit_cases as E
from oracle import oracle

CSRC = pathlib.Path(__file__).resolve().parent.parent / "transformer-lm_amd" / "csrc"


# ---------------------------------------------------------------------- the constants
def _source_constants():
    """every `constexpr <type> kName = <expression>;` of the two files, evaluated in order"""
    env: dict = {}
    for name in ("stage.h", "encode.hip"):
        for m in re.finditer(r"^\s*constexpr\s+(?:unsigned\s+long\s+long|unsigned|int|size_t|uint32_t)\s+(k\w+)\s*=\s*([^;]+);",
                             (CSRC / name).read_text(), flags=re.M):
            expr = re.sub(r"\((?:int|unsigned)\)", "", m.group(2))
            expr = re.sub(r"(?<=\d)(?:ULL|ull|u|U)\b", "", expr).replace("/", "//")
            try:
                env[m.group(1)] = eval(expr, {"__builtins__": {}}, dict(env))   # noqa: S307 (the project's own source)
            except Exception:   # an expression this test has no use for
                continue
    return env


def test_restated_constants_equal_the_source():
    env = _source_constants()
    for mine, (_file, theirs) in E.SOURCE_CONSTANTS.items():
        assert theirs in env, theirs
        assert getattr(E, mine) == env[theirs], (mine, theirs)
    assert (E.K_CHUNK, E.K_EMIT_PARTS, E.K_EMIT_IDS, E.K_EMIT_R, E.K_CUT_ROUND) == (16384, 2, 6144, 8, 2048)
    assert (E.K_ENC_INLINE, E.K_INLINE) == (15, 16)
    text = (CSRC / "encode.hip").read_text()
    # the split and the three branches, as the kernels write them
    assert text.count("const uint32_t r0 = (uint32_t)((unsigned long long)mc * part / kEmitParts);") == 2
    assert text.count("const uint32_t m = (uint32_t)((unsigned long long)mc * (part + 1) / kEmitParts) - r0;") == 2
    assert "if (m <= 256u * kEmitR) {" in text and "} else if (T <= kEmitIds) {" in text
    assert "for (uint32_t b = 0; b < m; b += 256) {" in text                       # ROUND_C
    assert "constexpr unsigned kPer = 16 / sizeof(OutT);" in text
    assert "(((16 - ((uintptr_t)(out + P) & 15)) & 15) / sizeof(OutT))" in text    # Plan.head
    assert "if (gp + 24 > n) {" in text                                            # load_word's byte path
    assert "const bool inl = len <= (size_t)kEncInline;" in text


def test_tokenizer_id_counts():
    """the arithmetic the cases rely on"""
    for w, n in [(" a", 1), (" ab", 1), (" abab", 2), ("ab", 1), (E.GH16, 1), (E.JK15, 1), (" xyz", 4), (" xab", 3),
                 (" abababx", 4), (E.xword(2048), 2048), (E.xword(2048, 5), 2043), (E.xword(E.LONG_WORD, 3), E.LONG_WORD - 3)]:
        assert E.word_ids(w.encode()) == n, w[:20]
    for n_bytes, w in E.ONE.items():
        assert len(w) == n_bytes and E.word_ids(w.encode()) == 1
    v, w = E.vocab(), E.wide_vocab()
    assert sorted(v.values()) == sorted(w.values()) and max(v) < 65536
    assert [i for i in w if i >= 65536] == [E.WIDE_ID] and w[E.WIDE_ID] == E.WIDE_BYTE.encode()
    assert {len(b) for b in v.values()} >= {15, 16, 17}
    for name, f in E.CASES.items():
        assert E.WIDE_BYTE not in f() and "\r" not in f() and f().isascii(), name


# ---------------------------------------------------------------------- the plans
@functools.lru_cache(maxsize=None)
def _plan(name):
    return E.plan_of(E.CASES[name]())


@functools.lru_cache(maxsize=None)
def _ids(name):
    return oracle.encode(E.vocab(), E.merges(), E.SPECIALS, E.CASES[name]())


@pytest.mark.parametrize("name", list(E.CASES))
def test_plan_counts_the_oracles_ids(name):
    p = _plan(name)
    assert int(p.cs[-1]) == len(_ids(name)) and int(p.T.sum()) == len(_ids(name))
    assert E.plan(E.CASES[name]()) == p.chunks()
    assert len(E.CASES[name]()) < (1 << 20) * 3 // 4


def test_path_a_edges():
    p = _plan("path_a_edges")
    a = p.path() == "a"
    for e, per in ((2, 8), (4, 4)):
        width = f"uint{8 * e}"
        head, res = p.head(e), p.P % per
        assert np.array_equal(head, (per - res) % per)
        for r in range(per):
            at = a & (res == r)
            h = (per - r) % per
            for what, T in (("head - 1", h - 1), ("head", h), ("head + 1", h + 1), ("head + kPer", h + per)):
                if T >= 0:
                    assert (at & (p.T == T)).any(), f"a path-(a) part with T == {what} at P = {r} (mod {per}), {width}"
            assert (at & (p.T > 0)).any(), f"a path-(a) part at P = {r} (mod {per}), {width}"
    for T in (0, 1, E.K_EMIT_IDS - 1, E.K_EMIT_IDS):
        assert (a & (p.T == T)).any(), f"a path-(a) part with T == {T}"
    assert (a & (p.T == 0) & (p.m == 0)).any(), "an empty part 0 (a chunk of one record)"
    assert (a & (p.T == E.K_EMIT_IDS) & (p.m == E.PART_RECORDS)).any(), "a path-(a) part at both limits, m 2048 and T 6144"
    assert ((p.path() == "b") & (p.m == 1)).any(), "a path-(b) part of one record"


def test_path_b():
    p = _plan("path_b")
    b = p.path() == "b"
    few = b & (p.m <= 8)
    assert (few & (p.T == E.K_EMIT_IDS + 1)).any(), "a path-(b) part of few records with T == 6145"
    assert (few & (p.T > 9500) & (p.T < 10500)).any(), "a path-(b) part of few records with T around 10 000"
    assert (b & (p.m == 1) & (p.T > E.K_EMIT_IDS)).any(), "a path-(b) part whose single word exceeds 6144 ids"
    assert (b & (p.m == E.PART_RECORDS) & (p.T == E.K_EMIT_IDS + 1)).any(), "a path-(b) part of 2048 records with T == 6145"
    # the pair made by one byte: chunks 0 and 1 have the same records, one word a byte longer
    assert (p.m[0], p.T[0], p.path()[0]) == (4, E.K_EMIT_IDS, "a") and (p.m[2], p.T[2], p.path()[2]) == (4, E.K_EMIT_IDS + 1, "b")
    t = E.path_b()
    w0 = [len(w) for w in t[:E.K_CHUNK].split(" ")[1:5]]
    w1 = [len(w) for w in t[E.K_CHUNK:2 * E.K_CHUNK].split(" ")[1:5]]
    assert sum(w1) - sum(w0) == 1 and sum(a != b for a, b in zip(w0, w1)) == 1
    assert ((p.path() == "a") & (p.T == E.K_EMIT_IDS)).sum() >= 2
    assert set((p.P[b] * 2 % 16).tolist()) >= {0, 2}, "path-(b) parts at an aligned and an unaligned uint16 address"


def test_records_edge():
    p = _plan("records_edge")
    path = p.path()
    for m in (2047, 2048):
        assert ((p.m == m) & (path == "a")).any(), f"a path-(a) part of {m} records"
    assert ((p.m == 2048) & (path == "b")).any(), "a path-(b) part of 2048 records"
    for m in (2049, 4096, 8192):
        assert ((p.m == m) & (path == "c")).any(), f"a path-(c) part of {m} records"
    c = np.flatnonzero(path == "c")
    assert any(p.T[j] == p.m[j] for j in c), "a path-(c) part of one-id records"
    several = [j for j in c if p.T[j] > p.m[j]]
    assert several, "a path-(c) part with records of several ids"
    for j in several:   # every round's total differs from 256: the running offset matters
        n = p.nids[p.lo[j]:p.lo[j] + p.m[j]]
        assert all(n[k:k + E.ROUND_C].sum() != E.ROUND_C for k in range(0, len(n) - E.ROUND_C, E.ROUND_C))
    lens = E.records(E.records_edge().encode())[1]
    assert set(lens[:E.K_CHUNK].tolist()) == {1} and set(lens[E.K_CHUNK:E.K_CHUNK + 8192].tolist()) == {2}
    # chunks 3 and 4: the chunk's count tuned so that the part lands on the value
    assert p.chunks()[3][0] == 4097 and p.chunks()[4][0] == 4095 and p.chunks()[6][0] == 4098


def test_empty_chunks():
    p = _plan("empty_chunks")
    mc = p.mc
    assert mc[1] == 0 and mc[2] == 0, "two chunks without a record (a word runs through them)"
    starts, lens, _n = E.records(E.empty_chunks().encode())
    k = int(np.argmax(lens))
    assert lens[k] == E.LONG_WORD and starts[k] % E.K_CHUNK > E.K_CHUNK - 1024, "a 40 KiB word that starts late in a chunk"
    ones = np.flatnonzero(mc == 1)
    assert len(ones) >= 2 and all(p.m[2 * c] == 0 and p.m[2 * c + 1] == 1 for c in ones), "chunks of one record: part 0 empty"
    data = E.empty_chunks().encode()
    first = [data[int(starts[p.lo[2 * c + 1]]):][:13] for c in ones]
    assert E.EOT.encode() in first, "a special as a chunk's only record"
    assert any(f[:3] == b" ab" for f in first), "a word as a chunk's only record"
    assert 0 < len(data) % E.K_CHUNK < 16 and mc[-1] > 0, "a last chunk of a few bytes"
    assert mc[3] > 0 and starts[p.lo[6]] > 3 * E.K_CHUNK, "the first record after the empty chunks lies inside chunk 3"


# ---------------------------------------------------------------------- workgroup reuse
def test_mixed_reuse_block():
    block = E.reuse_block()
    assert len(block) == E.BLOCK_BYTES == 3 * E.K_CHUNK + 8 and E.BLOCK_BYTES % E.K_CHUNK
    v, m = E.vocab(), E.merges()
    one = oracle.encode(v, m, E.SPECIALS, block)
    assert oracle.encode(v, m, E.SPECIALS, block * 2) == one * 2, "the ids of N blocks are a tiling"
    s1, l1, n1 = E.records(block.encode())
    s2, l2, n2 = E.records((block * 2).encode())
    assert np.array_equal(s2, np.concatenate([s1, s1 + E.BLOCK_BYTES])) and np.array_equal(n2, np.tile(n1, 2))
    assert max(one) < 65536
    p1 = E.plan_of(block)
    assert set(p1.path().tolist()) == {"a", "b", "c"}, "one block holds a part of every path"
    two = E.reuse_plan(2)
    assert two.chunks() == E.plan(block * 2)


def test_mixed_reuse_repetitions():
    reps = E.reuse_reps(E.NOMINAL_CUS)
    p = E.reuse_plan(reps)
    assert len(p.m) >= E.reuse_parts_needed(E.NOMINAL_CUS) == 5120
    assert 38 << 20 < reps * E.BLOCK_BYTES < 44 << 20
    path = p.path()
    for k in "abc":
        sel = (path == k) & (p.T > 0)
        assert sel.sum() > 200, f"path ({k}) over the repetitions"
        assert set((p.P[sel] % 8).tolist()) == set(range(8)), f"path ({k}) at every residue of P mod 8"
    # every repetition meets the chunk grid at another phase
    assert len({(r * E.BLOCK_BYTES) % E.K_CHUNK for r in range(reps)}) == reps
    for per_cu in range(1, E.MAX_WG_PER_CU + 1):   # whatever the occupancy: a workgroup's later parts take every path
        later = path[per_cu * E.NOMINAL_CUS * 2:]
        assert set(later.tolist()) == {"a", "b", "c"}, f"every path among a workgroup's later parts at {per_cu} workgroups per CU"


# ---------------------------------------------------------------------- word loads
def test_word_loads():
    text = E.word_loads()
    data = text.encode()
    starts, lens, _n = E.records(data)
    words = {(int(ln), int(s) % 8) for s, ln in zip(starts, lens) if data[s:s + 1] not in (b"\n", b"7")}
    for L in E.WORD_LENGTHS:
        for a in range(8):
            assert (L, a) in words, f"a word of {L} bytes whose first byte lies {a} past an 8-byte boundary"
    toks = {data[s:s + ln] for s, ln in zip(starts.tolist(), lens.tolist())}
    entries = set(E.vocab().values())
    for L in (2, 4, 8, 15, 16):
        assert any(len(t) == L and t in entries for t in toks), f"a vocab entry of {L} bytes as a pre-token"
        assert any(len(t) == L and t not in entries for t in toks), f"a pre-token of {L} bytes that is no vocab entry"
    assert any(len(t) == 17 and t in entries for t in toks) and any(len(t) == 17 and t not in entries for t in toks)
    for w in E.vocab_entry_words():
        assert w.encode() in entries or w in ("jk" * 7, "jk" * 4)
        for a in range(8):
            assert any(data[s:s + ln] == w.encode() and s % 8 == a for s, ln in zip(starts.tolist(), lens.tolist())), (w, a)
    for L in (E.K_ENC_INLINE, E.K_INLINE, E.K_INLINE + 1):
        same = [t for t in toks if len(t) == L and t not in entries]
        for k, what in ((0, "byte 0"), (7, "byte 7"), (8, "byte 8"), (L - 1, "the last byte")):
            assert any(sum(x != y for x, y in zip(a, b)) == 1 and a[k] != b[k] for a in same for b in same), \
                f"twins of {L} bytes that differ only in {what}"
    assert any(t[:15] in toks and t[:16] in toks for t in toks if len(t) == 17), "words of 15, 16, 17 bytes that differ only in length"
    for L in (17, 18, 24, 25, 33, 40):
        same = [t for t in toks if len(t) == L]
        assert any(a[:-1] == b[:-1] and a != b for a in same for b in same), f"twins of {L} bytes that differ only in the last byte"
    for k in range(1, 18):
        assert b"\x00" * k in toks, f"a word of {k} NUL bytes"
    assert (len(E.GH16), 0) in words


def test_word_load_tails():
    seen = set()
    for t in E.word_load_tails():
        data = t.encode()
        s, ln, after = E.last_word(data)
        seen.add((ln, after, s + 24 > len(data)))
    for d in E.TAIL_DISTANCES:
        for L in E.TAIL_LENGTHS:
            assert (L, d, L + d < 24) in seen, f"a last word of {L} bytes with {d} bytes after it"
    assert {True, False} == {byte_path for L, _d, byte_path in seen if L <= 16}, "both sides of gp + 24 > n for words load_word reads"
    assert any(L == 15 and d == 0 for L, d, _b in seen) and any(L == 16 and d == 8 for L, d, _b in seen)


# ---------------------------------------------------------------------- uint16 refusals
def test_refusal_placements():
    base = E.refusal_base()
    assert E.WIDE_BYTE not in base and len(base) == 4 * E.K_CHUNK
    pos = E.refusal_positions()
    assert set(pos) == set(E.REFUSAL_REGIONS)
    wide_ids = oracle.encode(E.wide_vocab(), E.merges(), E.SPECIALS, base)
    assert max(wide_ids) < 65536
    for region in E.REFUSAL_REGIONS:
        text = E.refusal_text(region)
        assert text.count(E.WIDE_BYTE) == 1
        ids = oracle.encode(E.wide_vocab(), E.merges(), E.SPECIALS, text)
        assert ids.count(E.WIDE_ID) == 1 and sum(i >= 65536 for i in ids) == 1
        k = ids.index(E.WIDE_ID)
        p = E.plan_of(text)
        assert p.chunks() == E.plan(base)
        got = p.region(k, 2)
        j = int(np.searchsorted(p.P, k, "right")) - 1
        if region == "head":
            assert got == "head" and p.head(2)[j] == 4 and p.path()[j] == "a", "the wide id in a head element"
        elif region == "body_even":
            assert got in ("body0", "body2", "body4", "body6"), "the wide id in the even slot of a packed pair"
        elif region == "body_odd":
            assert got in ("body1", "body3", "body5", "body7"), "the wide id in the odd slot of a packed pair"
        elif region == "tail":
            assert got == "tail" and (p.T[j] - p.head(2)[j]) % 8 == 4, "the wide id in a tail element"
        elif region == "b":
            assert got == "b" and p.path()[j] == "b", "the wide id in a path-(b) part"
        elif region == "c_first":
            assert got == "c0" and p.path()[j] == "c", "the wide id in the first round of a path-(c) part"
        else:
            assert got[0] == "c" and int(got[1:]) >= 1 and p.path()[j] == "c", "the wide id in a later round of a path-(c) part"
