"""errors="replace" / "ignore" on the device: the repair kernel against CPython's decoder, then
the same bytes through every entry point that reads text.

The oracle everywhere is CPython on the same bytes: raw.decode("utf-8", mode) for the kernel, the
text-mode read (TextIOWrapper, newline=None) for files, a counting error handler for the stats.
Every comparison is exact.  The case builders are in utf8_repair_cases.py and checked on the CPU
in test_utf8_repair_cases.py."""
import functools

import numpy as np
import pytest

import gpt2_files
import utf8_repair_cases as C
from oracle import oracle

pytestmark = pytest.mark.gpu

MODES = ("replace", "ignore")
W = 65536
EOT = "<|endoftext|>"
SPECIALS = [EOT]


def _amd():
    import bpe_amd
    return bpe_amd


@functools.lru_cache(maxsize=None)
def _geom():
    return _amd().utf8.repair_geometry()


@functools.lru_cache(maxsize=None)
def _exhaustive():
    return C.exhaustive_buffer()


@functools.lru_cache(maxsize=None)
def _want(raw, mode):
    return C.cpython_repair(raw, mode)


def _stats(st):
    return st["n_units"], st["n_bytes"], st["first"]


def _check(raw, mode):
    got, st = _amd().repair_utf8(raw, mode)
    assert got == C.cpython_repair(raw, mode)
    assert _stats(st) == C.cpython_stats(raw)
    return st


# ---------------------------------------------------------------- the kernel against CPython
@pytest.mark.parametrize("mode", MODES)
def test_exhaustive_strings(mode):
    raw = _exhaustive()
    got, st = _amd().repair_utf8(raw, mode)
    assert got == _want(raw, mode)
    assert _stats(st) == C.cpython_stats(raw)


@pytest.mark.parametrize("mode", MODES)
def test_seams(mode):
    unit, tile = _geom()
    n = 0
    for name, raw in C.seam_cases(unit, tile):
        got, st = _amd().repair_utf8(raw, mode)
        assert got == C.cpython_repair(raw, mode), name
        assert _stats(st) == C.cpython_stats(raw), name
        n += 1
    assert n == len(C.PATTERNS) * 40


def test_first_is_where_strict_mode_stops():
    bpe_amd = _amd()
    unit, tile = _geom()
    cases = [raw for _n, raw in C.seam_cases(unit, tile)][::7] + [C.all_seams_buffer(unit, tile)]
    with bpe_amd.WordCounter() as c:
        for raw in cases:
            _out, st = bpe_amd.repair_utf8(raw, "replace")
            if st["first"] is None:
                c.add_bytes(raw, errors="strict")
                continue
            with pytest.raises(UnicodeDecodeError) as e:
                c.add_bytes(raw, errors="strict")
            assert e.value.start == st["first"] == C.strict_position(raw)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("offset", [1, 5, 15])
def test_offset_device_pointers(offset, mode):
    import torch
    bpe_amd = _amd()
    unit, tile = _geom()
    for raw in (C.all_seams_buffer(unit, tile), _exhaustive()):
        base = torch.frombuffer(bytearray(b"\xbf" * offset + raw), dtype=torch.uint8).to("cuda")
        view = base[offset:]
        assert view.data_ptr() % 16 == offset and view.is_contiguous()
        out, st = bpe_amd.repair_utf8(view, mode)
        assert out.cpu().numpy().tobytes() == _want(raw, mode)
        assert _stats(st) == C.cpython_stats(raw)
        assert base.cpu().numpy().tobytes() == b"\xbf" * offset + raw   # the input is not modified


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [0, 1, 2, 3, 17])
def test_tiny_inputs(n, mode):
    fills = [b"\xff" * 17, b"\xf0\x9f\x98\x80" * 5, b"a" * 14 + b"\xf0\x9f\x98", b"\xe2\x82" + b"b" * 15,
             b"\x80" * 17, b"a" * 17]
    for f in fills:
        _check(f[:n], mode)


def test_all_ff_grows_threefold_and_empties():
    _unit, tile = _geom()
    raw = b"\xff" * (tile + 1)
    got, st = _amd().repair_utf8(raw, "replace")
    assert got == C.FFFD * (tile + 1) and _stats(st) == (tile + 1, tile + 1, 0)
    import torch
    t = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to("cuda")
    out, st = _amd().repair_utf8(t, "ignore")
    assert out.numel() == 0 and _stats(st) == (tile + 1, tile + 1, 0)
    assert _amd().repair_utf8(raw, "ignore")[0] == b""


@pytest.mark.parametrize("mode", MODES)
def test_well_formed_multibyte_text_is_unchanged(mode):
    raw = C.multibyte_text()
    got, st = _amd().repair_utf8(raw, mode)
    assert got == raw and _stats(st) == (0, 0, None)
    assert _amd().last_utf8_errors() == {"errors": mode, "n_units": 0, "n_bytes": 0, "first": None}


def test_output_offsets_past_4gib():
    """1 431 655 800 bytes of 0xFF in replace mode are 4 294 967 400 bytes of U+FFFD, past 2^32.
    The expectation is analytic: nothing this large goes through CPython."""
    import torch
    n = 1_431_655_800
    t = torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda")
    out, st = _amd().repair_utf8(t, "replace")
    del t
    assert out.numel() == 3 * n == 4_294_967_400 > 1 << 32
    assert _stats(st) == (n, n, 0)
    tri = out.view(-1, 3)
    for k, b in enumerate(C.FFFD):
        assert bool((tri[:, k] == b).all()), k


# ---------------------------------------------------------------- through the layers
@functools.lru_cache(maxsize=None)
def _dirty():
    return C.dirty_corpus((gpt2_files.FIXTURES / "corpus.en").read_bytes(), window=W)


@functools.lru_cache(maxsize=None)
def _clean():
    return (gpt2_files.FIXTURES / "corpus.en").read_bytes()[:100_000].rsplit(b" ", 1)[0]


@functools.lru_cache(maxsize=None)
def _text(raw, mode):
    """The bytes of the text a text-mode read with errors=mode gives."""
    return C.cpython_read(raw, mode).encode("utf-8")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("utf8")
    (d / "dirty.txt").write_bytes(_dirty())
    (d / "clean.txt").write_bytes(_clean())
    for i, v in enumerate(C.straddle_variants(_dirty(), W)):
        (d / f"straddle{i}.txt").write_bytes(v)
    return d


def _words(text, specials=()):
    return {w: n for w, n in oracle.word_counts(text, specials).items() if len(w) > 1}


@pytest.mark.parametrize("mode", MODES)
def test_word_counter(files, mode):
    import torch
    bpe_amd = _amd()
    raw, path = _dirty(), files / "dirty.txt"
    want = _words(_text(raw, mode))
    units, nbytes, first = C.cpython_stats(raw)
    report = {"errors": mode, "n_units": units, "n_bytes": nbytes}
    with bpe_amd.WordCounter() as c:
        assert c.add_file(path, window_bytes=W, errors=mode).counts() == want
        assert c.info()["n_windows"] >= 3
        assert bpe_amd.last_utf8_errors() == {**report, "first": (str(path), first)}
    with bpe_amd.WordCounter() as c:
        assert c.add_bytes(raw, errors=mode).counts() == want
        assert bpe_amd.last_utf8_errors() == {**report, "first": (None, first)}
    with bpe_amd.WordCounter() as c:
        t = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to("cuda")
        assert c.add_tensor(t, errors=mode).counts() == want
        assert t.cpu().numpy().tobytes() == raw
        assert bpe_amd.last_utf8_errors() == {**report, "first": (None, first)}


@pytest.mark.parametrize("mode", MODES)
def test_window_seams_of_the_counter(files, mode):
    bpe_amd = _amd()
    for i, raw in enumerate(C.straddle_variants(_dirty(), W)):
        want = _words(_text(raw, mode))
        with bpe_amd.WordCounter() as c:
            assert c.add_file(files / f"straddle{i}.txt", window_bytes=W, errors=mode).counts() == want
        with bpe_amd.WordCounter() as c:
            assert c.add_file(files / f"straddle{i}.txt", errors=mode).counts() == want   # one window


@pytest.mark.parametrize("mode", MODES)
def test_train(files, mode):
    bpe_amd = _amd()
    raw, path = _dirty(), files / "dirty.txt"
    want = oracle.train_raw(_text(raw, mode), 400, SPECIALS)
    assert bpe_amd.train_bpe(path, 400, SPECIALS, errors=mode) == want
    assert bpe_amd.last_utf8_errors()["n_units"] == C.cpython_stats(raw)[0]
    assert bpe_amd.train_bpe_bytes(raw, 400, SPECIALS, errors=mode) == want
    c = oracle.Counter(SPECIALS)
    for doc in (_text(raw, mode), _clean()):
        a = np.frombuffer(doc, dtype=np.uint8)
        c.feed(a.ctypes.data, a.size)
    want2 = c.train(400)
    c.close()
    assert bpe_amd.train_bpe_files([path, files / "clean.txt"], 400, SPECIALS, window_bytes=W, errors=mode) == want2
    assert bpe_amd.last_utf8_errors() == {"errors": mode, "n_units": C.cpython_stats(raw)[0],
                                          "n_bytes": C.cpython_stats(raw)[1],
                                          "first": (str(path), C.cpython_stats(raw)[2])}


def test_strict_add_file_leaves_the_counter_as_it_was(files):
    bpe_amd = _amd()
    with bpe_amd.WordCounter() as c:
        c.add_bytes(b"hello world hello", errors="strict")
        before = c.counts()
        with pytest.raises(UnicodeDecodeError) as e:
            c.add_file(files / "dirty.txt", window_bytes=W, errors="strict")
        assert e.value.start == C.strict_position(_dirty())
        assert c.counts() == before and c.info()["n_inputs"] == 1


@functools.lru_cache(maxsize=None)
def _gpt2():
    vocab, merges = gpt2_files.load_gpt2(SPECIALS)
    return vocab, merges, oracle.PieceEncoder(vocab, merges, SPECIALS)


@functools.lru_cache(maxsize=None)
def _tok():
    vocab, merges, _ = _gpt2()
    return _amd().Tokenizer(dict(vocab), list(merges), SPECIALS)


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_tokenizer():
    yield   # the cached tokenizer frees its device handle here, not at interpreter exit
    _tok.cache_clear()


@functools.lru_cache(maxsize=None)
def _piece_ids(raw, mode, k):
    """The oracle's encode of each k-character piece of the CPython-decoded text, concatenated."""
    data = np.frombuffer(_text(raw, mode), dtype=np.uint8)
    if data.size == 0:
        return np.zeros(0, dtype=np.uint32)
    starts = np.flatnonzero((data & 0xC0) != 0x80)[::k]
    return _gpt2()[2].encode(data.ctypes.data, data.size, starts.astype(np.uint64))


def _encode_files(paths, tmp_path, k, mode, **kw):
    out = tmp_path / "out.bin"
    res = _amd().encode_files(_tok(), paths, out, chars_per_piece=k, errors=mode, **kw)
    ids = np.fromfile(out, dtype=res["dtype"])
    assert ids.size == res["n_ids"]
    return res, ids


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [7, 1_048_576])
def test_encode_files(files, tmp_path, k, mode):
    bpe_amd = _amd()
    dirty, clean = files / "dirty.txt", files / "clean.txt"
    want = [_piece_ids(_dirty(), mode, k), _piece_ids(_clean(), mode, k), _piece_ids(_dirty(), mode, k)]
    res, ids = _encode_files([dirty, clean, dirty], tmp_path, k, mode, window_bytes=W)
    assert np.array_equal(ids, np.concatenate(want))
    units, nbytes, first = C.cpython_stats(_dirty())
    assert res["file_replaced"].dtype == np.int64 and res["file_replaced"].tolist() == [units, 0, units]
    assert res["n_replaced"] == 2 * units
    assert res["file_offsets"].tolist() == [0] + np.cumsum([w.size for w in want]).tolist()
    assert res["n_windows"] >= 3 + 2 + 3
    assert bpe_amd.last_utf8_errors() == {"errors": mode, "n_units": 2 * units, "n_bytes": 2 * nbytes,
                                          "first": (str(dirty), first)}
    # the window-seam check: one window per file gives the same stream
    res1, ids1 = _encode_files([dirty, clean, dirty], tmp_path, k, mode)
    assert np.array_equal(ids1, ids) and res1["file_replaced"].tolist() == [units, 0, units]
    # encode_file and encode_bytes_u16 give the first file's ids
    assert np.array_equal(bpe_amd.encode.encode_file(_tok(), dirty, chars_per_piece=k, errors=mode), want[0])
    assert bpe_amd.last_utf8_errors()["first"] == (str(dirty), first)
    assert np.array_equal(bpe_amd.encode.encode_bytes_u16(_tok(), _dirty(), chars_per_piece=k, errors=mode), want[0])


@pytest.mark.parametrize("mode", MODES)
def test_window_seams_of_encode_files(files, tmp_path, mode):
    for i, raw in enumerate(C.straddle_variants(_dirty(), W)):
        want = _piece_ids(raw, mode, 1000)
        res, ids = _encode_files([files / f"straddle{i}.txt"], tmp_path, 1000, mode, window_bytes=W)
        assert np.array_equal(ids, want), i
        assert res["file_replaced"].tolist() == [C.cpython_stats(raw)[0]]


def test_strict_encode_files_result_has_todays_keys(files, tmp_path):
    out = tmp_path / "o.bin"
    res = _amd().encode_files(_tok(), [files / "clean.txt"], out, errors="strict")
    assert "n_replaced" not in res and "file_replaced" not in res
    with pytest.raises(UnicodeDecodeError):
        _amd().encode_files(_tok(), [files / "dirty.txt"], tmp_path / "p.bin", errors="strict")
    assert not (tmp_path / "p.bin").exists()


def test_clean_input_is_the_same_in_every_mode(files, tmp_path):
    bpe_amd = _amd()
    raw, path = _clean(), files / "clean.txt"
    out, st = bpe_amd.repair_utf8(raw, "replace")
    assert out == raw and _stats(st) == (0, 0, None)
    strict = bpe_amd.train_bpe(path, 400, SPECIALS, errors="strict")
    assert bpe_amd.train_bpe(path, 400, SPECIALS, errors="replace") == strict
    assert bpe_amd.last_utf8_errors() == {"errors": "replace", "n_units": 0, "n_bytes": 0, "first": None}
    ids_strict = bpe_amd.encode.encode_file(_tok(), path, errors="strict")
    assert np.array_equal(bpe_amd.encode.encode_file(_tok(), path, errors="replace"), ids_strict)
    res_s = bpe_amd.encode_files(_tok(), [path], tmp_path / "s.bin", window_bytes=W, errors="strict")
    res_r = bpe_amd.encode_files(_tok(), [path], tmp_path / "r.bin", window_bytes=W, errors="replace")
    assert (tmp_path / "s.bin").read_bytes() == (tmp_path / "r.bin").read_bytes()
    assert res_r["n_replaced"] == 0 and res_r["n_ids"] == res_s["n_ids"] == ids_strict.size
