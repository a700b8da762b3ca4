"""The dataset encoder bpe_amd.encode_files and the device helpers id_counts / id_positions.

The expected stream never comes from the code under test.  For each file: Python's own text-mode
read gives the text, the byte offset of every chars_per_piece-th character gives the cuts, and the
oracle's PieceEncoder encodes each piece on its own.  Where the file is small the parent path
encode_file(tok, p) on the same file is a second, independent check.

Windows are 64 KiB (the minimum) and the read grid is fixed, so every hazard is placed on it: the
range ends at W, 2W, ... of the raw file.
"""
import functools
import os
import random

import numpy as np
import pytest

import gpt2_files
from oracle import oracle

pytestmark = pytest.mark.gpu

W = 65536
EOT = "<|endoftext|>"
SPECIALS = [EOT]
FRAGMENTS = ["the", " cat", "été", " naïve", EOT, "\n", "\r\n", "  ", "12", "'s", "!!", " 東京", "—", " x" * 3, "\t",
             "ab<|end", "oftext|>cd", " 😀", "\r"]


@functools.lru_cache(maxsize=None)
def _gpt2():
    vocab, merges = gpt2_files.load_gpt2(SPECIALS)
    return vocab, merges, oracle.PieceEncoder(vocab, merges, SPECIALS)


@functools.lru_cache(maxsize=None)
def _tok():
    from bpe_amd import Tokenizer
    vocab, merges, _ = _gpt2()
    return Tokenizer(dict(vocab), list(merges), SPECIALS)


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_tokenizers():
    yield   # the cached tokenizers free their device handles here, not at interpreter exit
    _tok.cache_clear()
    _wide.cache_clear()


def _sep_id():
    return _tok().vocab_inv[EOT.encode()]


def _mixed(seed: int, n_bytes: int, fragments=FRAGMENTS) -> bytes:
    """Raw file bytes of about n_bytes built from the fragments (whole fragments: valid UTF-8)."""
    rng = random.Random(seed)
    parts, size = [], 0
    while size < n_bytes:
        f = rng.choice(fragments).encode("utf-8")
        parts.append(f)
        size += len(f)
    return b"".join(parts)


def _no_cr(seed, n_bytes):
    return _mixed(seed, n_bytes, [f for f in FRAGMENTS if "\r" not in f])


def _place(data: bytes, at: int, hazard: bytes, inner: int) -> bytes:
    """data with `hazard` spliced in so that the range end `at` falls after its first `inner` bytes
    (the filler before it is cut at a character and padded with 'x')."""
    start = at - inner
    cut = start
    while cut > 0 and (data[cut] & 0xC0) == 0x80:
        cut -= 1
    return data[:cut] + b"x" * (start - cut) + hazard + data[cut:]


def _expected(path, k: int, enc=None) -> np.ndarray:
    enc = enc or _gpt2()[2]
    with open(path, "r", encoding="utf-8") as f:
        text = f.read()
    data = np.frombuffer(text.encode("utf-8"), dtype=np.uint8)
    if data.size == 0:
        return np.zeros(0, dtype=np.uint32)
    starts = np.flatnonzero((data & 0xC0) != 0x80)[::k]
    return enc.encode(data.ctypes.data, data.size, starts.astype(np.uint64))


def _write(tmp_path, name, raw: bytes):
    p = tmp_path / name
    p.write_bytes(raw)
    return p


def _run(paths, tmp_path, k, **kw):
    import bpe_amd
    out = tmp_path / "out.bin"
    kw.setdefault("window_bytes", W)
    res = bpe_amd.encode_files(_tok(), paths, out, chars_per_piece=k, **kw)
    ids = np.fromfile(out, dtype=res["dtype"])
    assert ids.size == res["n_ids"]
    return res, ids


def _check_files(paths, tmp_path, k, **kw):
    want = [_expected(p, k) for p in paths]
    res, ids = _run(paths, tmp_path, k, **kw)
    cat = np.concatenate(want) if want else np.zeros(0, np.uint32)
    assert res["dtype"] == np.uint16
    assert np.array_equal(ids.astype(np.uint32), cat)
    assert res["file_offsets"].dtype == np.int64
    assert res["file_offsets"].tolist() == np.concatenate([[0], np.cumsum([w.size for w in want])]).tolist()
    sizes = [os.path.getsize(p) for p in paths]
    assert res["n_bytes"] == sum(sizes)
    assert res["n_windows"] == sum(-(-s // W) for s in sizes)
    return res, ids, cat


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("k", [997, 4096, 100_000])
def test_parity_with_oracle_and_parent(tmp_path, k):
    from bpe_amd.encode import encode_file
    p = _write(tmp_path, "mixed.txt", _mixed(11, 300 * 1024))
    res, ids, want = _check_files([p], tmp_path, k)
    assert np.array_equal(encode_file(_tok(), p, chars_per_piece=k), ids)
    assert res["max_window_bytes"] == W and res["device_bytes"] > 2 * W
    with open(p, "r", encoding="utf-8") as f:
        n_chars = len(f.read())
    assert res["n_pieces"] == -(-n_chars // k)
    if k == 100_000:   # a piece of 100 000 characters is longer than a window: the buffer grew
        assert res["n_grows"] >= 1


# ------------------------------------------------------------------ hazards on the read grid
HAZARDS = [
    ("cr_last_byte", b"\rA", 1),
    ("crlf_split", b"\r\n", 1),
    ("crcrlf_1", b"\r\r\n", 1),
    ("crcrlf_2", b"\r\r\n", 2),
    ("char2_1", "é".encode(), 1),
    ("char3_1", "東".encode(), 1),
    ("char3_2", "東".encode(), 2),
    ("char4_1", "😀".encode(), 1),
    ("char4_2", "😀".encode(), 2),
    ("char4_3", "😀".encode(), 3),
    ("special_split_by_window", EOT.encode(), 6),
    ("special_after_cr", b"\r" + EOT.encode(), 1),
]


@pytest.mark.parametrize("name,hazard,inner", HAZARDS, ids=[h[0] for h in HAZARDS])
def test_hazard_alone_on_the_grid(tmp_path, name, hazard, inner):
    base = _no_cr(21, 200 * 1024)
    if name == "special_split_by_window":
        # ASCII without any other special, so characters are bytes: the pieces start at multiples
        # of 997, none of them inside the special at [W - 6, W + 7)
        base = b"ab cd " * (200 * 1024 // 6)
    raw = _place(base, W, hazard, inner)
    assert raw[W - inner:W - inner + len(hazard)] == hazard
    p = _write(tmp_path, "h.txt", raw)
    res, ids, want = _check_files([p], tmp_path, 997)
    if name == "special_split_by_window":   # a window edge is not a piece edge: the special is matched
        assert (want == _sep_id()).sum() == 1 and (ids == _sep_id()).sum() == 1


def test_all_hazards_in_one_file(tmp_path):
    raw = _no_cr(22, (len(HAZARDS) + 2) * W)
    for i, (_, hazard, inner) in enumerate(HAZARDS):
        raw = _place(raw, (i + 1) * W, hazard, inner)
    for i, (_, hazard, inner) in enumerate(HAZARDS):
        at = (i + 1) * W - inner
        assert raw[at:at + len(hazard)] == hazard
    p = _write(tmp_path, "all.txt", raw)
    for k in (997, 4096):
        _check_files([p], tmp_path, k)


def test_special_split_by_a_piece_edge_is_not_matched(tmp_path):
    k = 997
    # ASCII only, so characters are bytes: pieces start at multiples of k; one special lies across
    # the piece edge at 70 * k (and across no window edge), one lies whole inside a piece
    body = bytearray(b"ab cd " * (150 * 1024 // 6))
    eot = EOT.encode()
    edge = 70 * k
    body[edge - 5:edge - 5 + len(eot)] = eot
    body[edge + 300:edge + 300 + len(eot)] = eot
    p = _write(tmp_path, "edge.txt", bytes(body))
    res, ids, want = _check_files([p], tmp_path, k)
    assert (want == _sep_id()).sum() == 1


@pytest.mark.parametrize("size", [W - 1, W, W + 1])
def test_file_sizes_around_a_window(tmp_path, size):
    raw = _mixed(31, size + 64)
    cut = size
    while (raw[cut] & 0xC0) == 0x80:
        cut -= 1
    raw = raw[:cut] + b"y" * (size - cut)
    assert len(raw) == size
    res, _, _ = _check_files([_write(tmp_path, "s.txt", raw)], tmp_path, 997)
    assert res["n_windows"] == (2 if size > W else 1)


def test_file_that_ends_in_cr(tmp_path):
    for size in (W, W + 1, 3 * W + 77):
        raw = _no_cr(32, size)[:size - 1]
        while (raw[-1] & 0xC0) == 0x80 or raw[-1] >= 0xC0:
            raw = raw[:-1]
        raw = raw + b"z" * (size - 1 - len(raw)) + b"\r"
        assert len(raw) == size
        _check_files([_write(tmp_path, "cr.txt", raw)], tmp_path, 4096)


# ------------------------------------------------------------------ several files
def test_several_files(tmp_path):
    paths = [
        _write(tmp_path, "empty.txt", b""),
        _write(tmp_path, "one.txt", b"a"),
        _write(tmp_path, "small.txt", _mixed(41, 20_000)),
        _write(tmp_path, "empty2.txt", b""),
        _write(tmp_path, "many.txt", _mixed(42, 5 * W + 1234)),
        _write(tmp_path, "sep_first.txt", EOT.encode() + _mixed(43, 1000)),
    ]
    idx = tmp_path / "out.idx"
    res, ids, want = _check_files(paths, tmp_path, 4096, separator=EOT, index_path=idx, count_ids=True)
    assert np.array_equal(np.fromfile(idx, np.uint64), np.flatnonzero(want == _sep_id()))
    assert want[res["file_offsets"][5]] == _sep_id()   # a separator as the first id of a file
    size = max(_tok().vocab) + 1
    assert res["id_counts"].dtype == np.uint64 and res["id_counts"].size == size
    assert np.array_equal(res["id_counts"], np.bincount(want, minlength=size).astype(np.uint64))
    assert res["n_separators"] == (want == _sep_id()).sum()


def test_empty_paths(tmp_path):
    res, ids = _run([], tmp_path, 997, separator=EOT, index_path=tmp_path / "e.idx", count_ids=True)
    assert ids.size == 0 and res["n_ids"] == 0 and res["n_windows"] == 0 and res["n_bytes"] == 0
    assert res["file_offsets"].tolist() == [0]
    assert (tmp_path / "e.idx").read_bytes() == b"" and not res["id_counts"].any()


def test_fifo_input(tmp_path):
    import threading
    raw = _mixed(44, 100_000)
    ref = _write(tmp_path, "ref.txt", raw)
    fifo = tmp_path / "pipe"
    os.mkfifo(fifo)
    # A read end of our own, never read from: with it the writer's open returns at once, and
    # closing it wakes a writer that no one reads from (EPIPE).  So a call that fails before it
    # opens the FIFO cannot leave the writer thread, and with it this test, waiting.
    keep = os.open(fifo, os.O_RDONLY | os.O_NONBLOCK)

    def feed():
        fd = os.open(fifo, os.O_WRONLY)
        try:
            done = 0
            while done < len(raw):
                done += os.write(fd, raw[done:])
        except BrokenPipeError:
            pass   # nobody read: the test fails on its own assertions
        finally:
            os.close(fd)

    t = threading.Thread(target=feed, daemon=True)
    t.start()
    try:
        res, ids = _run([fifo], tmp_path, 997)
    finally:
        os.close(keep)
        t.join(30)
    assert not t.is_alive()
    assert np.array_equal(ids.astype(np.uint32), _expected(ref, 997))


# ------------------------------------------------------------------ wide ids
WIDE_ID = 70_000


@functools.lru_cache(maxsize=None)
def _wide():
    """GPT-2 plus a special <|doc|> at id 70 000.  The oracle runs on the dense vocab (the special
    at the next free id), and its ids are mapped to the sparse vocab here."""
    from bpe_amd import Tokenizer
    specials = [EOT, "<|doc|>"]
    dense, merges = gpt2_files.load_gpt2(specials)
    dense_id = max(dense)
    assert dense[dense_id] == b"<|doc|>"
    sparse = dict(dense)
    del sparse[dense_id]
    sparse[WIDE_ID] = b"<|doc|>"
    return Tokenizer(sparse, list(merges), specials), oracle.PieceEncoder(dense, merges, specials), dense_id


def test_wide_ids(tmp_path):
    import bpe_amd
    tok, enc, dense_id = _wide()
    raw = _mixed(51, 200 * 1024, FRAGMENTS + ["<|doc|>", " <|doc|>\n"])
    raw = _place(raw, 2 * W, b"<|doc|>", 3)
    p = _write(tmp_path, "wide.txt", raw)
    want = _expected(p, 4096, enc)
    want[want == dense_id] = WIDE_ID
    out, idx = tmp_path / "w.bin", tmp_path / "w.idx"
    res = bpe_amd.encode_files(tok, [p], out, window_bytes=W, chars_per_piece=4096, separator="<|doc|>", index_path=idx,
                               count_ids=True)
    assert res["dtype"] == np.uint32
    assert np.array_equal(np.fromfile(out, np.uint32), want)
    assert np.array_equal(np.fromfile(idx, np.uint64), np.flatnonzero(want == WIDE_ID))
    assert np.array_equal(res["id_counts"], np.bincount(want, minlength=WIDE_ID + 1).astype(np.uint64))
    # forced uint16: refused, never a wrapped id, and nothing is left behind
    for pre in (False, True):
        o16, i16 = tmp_path / "w16.bin", tmp_path / "w16.idx"
        if pre:
            o16.write_bytes(b"old tokens")
            i16.write_bytes(b"old index")
        with pytest.raises(RuntimeError):
            bpe_amd.encode_files(tok, [p], o16, dtype=np.uint16, window_bytes=W, chars_per_piece=4096,
                                 separator="<|doc|>", index_path=i16)
        if pre:
            assert o16.read_bytes() == b"old tokens" and i16.read_bytes() == b"old index"
        else:
            assert not o16.exists() and not i16.exists()
        assert sorted(x.name for x in tmp_path.iterdir() if ".tmp" in x.name) == []
    # a text without the wide special still fits uint16 when it is forced
    p2 = _write(tmp_path, "narrow.txt", _mixed(52, 3 * W))
    res = bpe_amd.encode_files(tok, [p2], out, dtype=np.uint16, window_bytes=W, chars_per_piece=4096)
    assert np.array_equal(np.fromfile(out, np.uint16).astype(np.uint32), _expected(p2, 4096, enc))


# ------------------------------------------------------------------ errors
def _error_cases(tmp_path):
    good = _no_cr(61, 3 * W)
    bad = bytearray(good)
    bad[W + 5:W + 6] = b"\xff"
    yield "bad_byte", [_write(tmp_path, "good.txt", good), _write(tmp_path, "bad.txt", bytes(bad))], UnicodeDecodeError
    yield "bad_continuation_over_the_edge", [_write(tmp_path, "edge.txt", _place(good, W, b"\xe6\x9dA", 2))], \
        UnicodeDecodeError
    trunc = good[:2 * W + 10]
    while (trunc[-1] & 0xC0) == 0x80 or trunc[-1] >= 0xC0:
        trunc = trunc[:-1]
    yield "truncated_at_eof", [_write(tmp_path, "trunc.txt", trunc + "東".encode()[:2])], UnicodeDecodeError
    yield "missing_second", [_write(tmp_path, "first.txt", good), tmp_path / "nothing_here.txt"], FileNotFoundError


@pytest.mark.parametrize("preexisting", [False, True], ids=["absent", "sentinels"])
def test_errors_leave_the_outputs_as_they_were(tmp_path, preexisting):
    import bpe_amd
    for name, paths, exc in _error_cases(tmp_path):
        out, idx = tmp_path / f"{name}.bin", tmp_path / f"{name}.idx"
        if preexisting:
            out.write_bytes(b"sentinel tokens " + name.encode())
            idx.write_bytes(b"sentinel index " + name.encode())
        with pytest.raises(exc) as ei:
            bpe_amd.encode_files(_tok(), paths, out, window_bytes=W, chars_per_piece=997, separator=EOT,
                                 index_path=idx, count_ids=True)
        if exc is UnicodeDecodeError:
            with pytest.raises(UnicodeDecodeError) as py:
                with open(paths[-1], "r", encoding="utf-8") as f:
                    f.read()
            assert ei.value.start == py.value.start, name
            assert os.fspath(paths[-1]) in str(ei.value)
            # the same number encode_file reports for that file
            with pytest.raises(UnicodeDecodeError) as parent:
                bpe_amd.encode.encode_file(_tok(), paths[-1], chars_per_piece=997)
            assert parent.value.start == ei.value.start
        if preexisting:
            assert out.read_bytes() == b"sentinel tokens " + name.encode()
            assert idx.read_bytes() == b"sentinel index " + name.encode()
        else:
            assert not out.exists() and not idx.exists()
        assert [x.name for x in tmp_path.iterdir() if ".tmp" in x.name] == []


# ------------------------------------------------------------------ separator index
def _sep_texts():
    none = _mixed(71, 3 * W, [f for f in FRAGMENTS if "endoftext" not in f and "<|" not in f and "|>" not in f])
    yield "none", none
    yield "begins_and_ends", EOT.encode() + none[:2 * W + 100].decode("utf-8", "ignore").encode() + EOT.encode()
    yield "runs", _mixed(72, 3 * W, [EOT * 3, EOT, " a", "\n", EOT * 7, " word"])
    yield "only_separators", EOT.encode() * (300 * 1024 // len(EOT))
    # the special ends exactly at a window edge and the next one starts the next range
    yield "first_id_of_a_window", _place(none, W, EOT.encode() * 2, len(EOT))


@pytest.mark.parametrize("pos_cap", [None, 1000], ids=["default", "small_position_buffer"])
def test_separator_index(tmp_path, monkeypatch, pos_cap):
    if pos_cap:   # a region's matches exceed the position buffer: it is searched in parts
        monkeypatch.setenv("BPE355_DS_POS_CAP", str(pos_cap))
    for name, raw in _sep_texts():
        p = _write(tmp_path, name + ".txt", raw)
        idx = tmp_path / (name + ".idx")
        res, ids, want = _check_files([p], tmp_path, 4096, separator=EOT, index_path=idx)
        pos = np.fromfile(idx, np.uint64)
        assert np.array_equal(pos, np.flatnonzero(want == _sep_id())), name
        assert res["n_separators"] == pos.size
        if name == "none":
            assert pos.size == 0
        if name == "only_separators":
            # (a piece edge inside a special unmatches it: not quite every id is a separator)
            assert pos.size > 23_000 and want.size - pos.size < 1000
    # an int id as the separator
    idx = tmp_path / "int.idx"
    res, ids, want = _check_files([p], tmp_path, 4096, separator=int(want[0]), index_path=idx)
    assert np.array_equal(np.fromfile(idx, np.uint64), np.flatnonzero(want == want[0]))


# ------------------------------------------------------------------ counts, bookkeeping
def test_count_ids_over_several_files(tmp_path):
    paths = [_write(tmp_path, f"c{i}.txt", _mixed(80 + i, n)) for i, n in enumerate((3 * W + 5, 1000, 2 * W))]
    res, ids, want = _check_files(paths, tmp_path, 997, count_ids=True)
    size = max(_tok().vocab) + 1
    assert np.array_equal(res["id_counts"], np.bincount(want, minlength=size).astype(np.uint64))


def test_default_window_writes_the_same_bytes(tmp_path):
    import bpe_amd
    paths = [_write(tmp_path, "d0.txt", _mixed(91, 4 * W + 99)), _write(tmp_path, "d1.txt", _mixed(92, 70_000))]
    res, ids, want = _check_files(paths, tmp_path, 4096)
    assert res["n_windows"] == 5 + 2 and res["max_window_bytes"] == W and res["device_bytes"] > 0
    for key in ("read_ms", "decode_ms", "encode_ms", "write_ms", "n_pieces", "n_separators"):
        assert key in res
    small = (tmp_path / "out.bin").read_bytes()
    out2 = tmp_path / "out_default.bin"
    res2 = bpe_amd.encode_files(_tok(), paths, out2, chars_per_piece=4096)
    assert out2.read_bytes() == small
    assert res2["n_windows"] == 2 and res2["max_window_bytes"] == 4 * W + 99
    assert res2["file_offsets"].tolist() == res["file_offsets"].tolist()


# ------------------------------------------------------------------ the kernels on id tensors
def _dev(a: np.ndarray):
    import torch
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)
    if a.dtype == np.uint32:
        return torch.from_numpy(a.view(np.int32)).cuda()
    return torch.from_numpy(a).cuda()


def _counts_host(t):
    import torch
    return t.view(torch.int64).cpu().numpy().view(np.uint64)


@functools.lru_cache(maxsize=None)
def _id_streams():
    rng = np.random.default_rng(5)
    zipf = np.minimum(rng.zipf(1.2, 1 << 20), 50_256).astype(np.uint16)
    return {
        "equal": np.full(1 << 20, 77, dtype=np.uint16),
        "uniform": rng.integers(0, 100_000, 1 << 20, dtype=np.uint32),
        "zipf": zipf,
    }


@pytest.mark.parametrize("name", ["equal", "uniform", "zipf"])
def test_id_counts_streams(name, monkeypatch):
    import bpe_amd
    a = _id_streams()[name]
    size = 100_000 if a.dtype == np.uint32 else 65_536
    want = np.bincount(a, minlength=size).astype(np.uint64)
    assert np.array_equal(_counts_host(bpe_amd.id_counts(_dev(a), size)), want)
    if a.dtype == np.uint16:   # int16 bits are read as unsigned; int64 holds the same ids
        import torch
        assert np.array_equal(_counts_host(bpe_amd.id_counts(_dev(a).view(torch.int16), size)), want)
        assert np.array_equal(_counts_host(bpe_amd.id_counts(_dev(a.astype(np.int64)), size)), want)
    # the bound on the ids a workgroup counts between two flushes of its private table, made small
    monkeypatch.setenv("BPE355_HIST_FLUSH_IDS", "5000")
    assert np.array_equal(_counts_host(bpe_amd.id_counts(_dev(a), size)), want)


def test_id_counts_offsets_and_ragged_lengths():
    import bpe_amd
    a = _id_streams()["zipf"][:100_003]
    t = _dev(a)
    for sl in (slice(1, None), slice(3, -5), slice(7, 8), slice(2, 2), slice(5, 12), slice(0, 17)):
        got = _counts_host(bpe_amd.id_counts(t[sl], 65_536))
        assert np.array_equal(got, np.bincount(a[sl], minlength=65_536).astype(np.uint64)), sl
    t32 = _dev(a.astype(np.uint32))
    for sl in (slice(1, None), slice(3, -5), slice(2, 5)):
        got = _counts_host(bpe_amd.id_counts(t32[sl], 65_536))
        assert np.array_equal(got, np.bincount(a[sl], minlength=65_536).astype(np.uint64)), sl


def test_id_counts_empty_out_of_range_and_64_bit_sum():
    import torch
    import bpe_amd
    assert not _counts_host(bpe_amd.id_counts(_dev(np.zeros(0, np.uint16)), 10)).any()
    a = np.array([3, 9, 500, 4, 70, 499, 9], dtype=np.uint32)
    with pytest.raises(ValueError, match=r"\b70\b"):
        bpe_amd.id_counts(_dev(a), 70)
    with pytest.raises(ValueError):
        bpe_amd.id_counts(_dev(np.array([1, -2, 3], dtype=np.int64)), 70)
    with pytest.raises(ValueError):
        bpe_amd.id_counts(_dev(np.array([1, 1 << 32, 3], dtype=np.int64)), 70)
    # out += counts, exact in 64 bits where a 32-bit cell would wrap
    out = torch.zeros(100, dtype=torch.int64, device="cuda")
    out[77] = (1 << 32) - 7
    out[5] = 1 << 40
    got = bpe_amd.id_counts(_dev(_id_streams()["equal"]), 100, out=out.view(torch.uint64))
    host = _counts_host(got)
    assert host[77] == (1 << 32) - 7 + (1 << 20) and host[5] == 1 << 40 and host.sum() == host[77] + host[5]


def test_id_positions():
    import torch
    import bpe_amd
    n = 1 << 20
    eq = _dev(_id_streams()["equal"])
    assert bpe_amd.id_positions(eq, 78).numel() == 0
    got = bpe_amd.id_positions(eq, 77)
    assert got.dtype == torch.int64 and torch.equal(got, torch.arange(n, device="cuda"))
    assert torch.equal(bpe_amd.id_positions(eq, 77, base=1 << 40), torch.arange(n, device="cuda") + (1 << 40))
    # matches only in the unaligned head and tail of a view that starts at an odd element
    a = np.zeros(100_001, dtype=np.uint16)
    view = slice(3, 100_001 - 2)
    hits = [0, 1, 4, 99_990, 99_995]
    for h in hits:
        a[3 + h] = 9
    a[0] = a[2] = a[-1] = 9   # outside the view
    t = _dev(a)[view]
    assert bpe_amd.id_positions(t, 9).tolist() == hits
    assert bpe_amd.id_positions(t, 9, base=1000).tolist() == [1000 + h for h in hits]
    for dt in (np.uint32, np.int64):
        z = _id_streams()["zipf"][:300_007].astype(dt)
        for sl in (slice(None), slice(1, -1), slice(3, 40)):
            got = bpe_amd.id_positions(_dev(z)[sl], 2, base=5).cpu().numpy()
            assert np.array_equal(got, np.flatnonzero(z[sl] == 2) + 5), (dt, sl)
    assert bpe_amd.id_positions(_dev(np.zeros(0, np.uint16)), 0).numel() == 0
    assert bpe_amd.id_positions(_dev(np.array([1, 2], np.uint16)), 70_000).numel() == 0
    with pytest.raises(ValueError):
        bpe_amd.id_positions(_dev(np.array([1, -1], dtype=np.int64)), 1)
