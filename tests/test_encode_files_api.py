"""CPU: the dataset encoder's argument checks (bpe_amd.encode_files raises ValueError before the
device is touched) and its carry rule, bpe_window_holdback, over every tail of 1-4 bytes drawn from
a set that holds ASCII, \\r, \\n and lead and continuation bytes of 2-, 3- and 4-byte characters.

The comparator of the carry rule is CPython's own decoder: a byte string is a proper prefix of a
well-formed sequence exactly when decoding it fails at offset 0 with "unexpected end of data".
"""
import ctypes
import itertools

import numpy as np
import pytest

import bpe_amd
from bpe_amd import _lib

ALPHABET = (0x41, 0x0D, 0x0A, 0xC3, 0xA9, 0xE6, 0x9D, 0xF0, 0x9F, 0x80)


def _tok():
    vocab = {i: bytes([i]) for i in range(256)}
    vocab[256] = b"<|endoftext|>"
    return bpe_amd.Tokenizer(vocab, [], ["<|endoftext|>"])


def _proper_prefix(b: bytes) -> bool:
    try:
        b.decode("utf-8")
    except UnicodeDecodeError as e:
        return e.start == 0 and e.reason == "unexpected end of data"
    return False


def _want_holdback(tail: bytes, at_eof: bool) -> int:
    if at_eof:
        return 0
    for k in (3, 2, 1):
        if k <= len(tail) and _proper_prefix(tail[-k:]):
            return k
    return 1 if tail[-1] == 0x0D else 0


def test_window_holdback_exhaustive():
    L = _lib.lib()
    wrong = []
    n_cases = 0
    for n in (1, 2, 3, 4):
        for t in itertools.product(ALPHABET, repeat=n):
            tail = bytes(t)
            for eof in (0, 1):
                n_cases += 1
                got = L.bpe_window_holdback(tail, n, eof)
                if got != _want_holdback(tail, bool(eof)):
                    wrong.append((tail.hex(), eof, got))
    assert n_cases == 2 * (10 + 100 + 1000 + 10000)
    assert not wrong, wrong[:10]


def test_window_holdback_looks_at_the_last_four_bytes_only():
    L = _lib.lib()
    assert L.bpe_window_holdback(b"\xf0\x9f\x80AAAA\xe6\x9d", 9, 0) == 2
    assert L.bpe_window_holdback(b"AAAAAAA\r", 8, 0) == 1
    assert L.bpe_window_holdback(b"AAAAAAA\r", 8, 1) == 0
    assert L.bpe_window_holdback(None, 0, 0) == 0
    # surrogates and overlong forms are not prefixes of anything well-formed
    assert L.bpe_window_holdback(b"\xed\xa0", 2, 0) == 0
    assert L.bpe_window_holdback(b"\xe0\x80", 2, 0) == 0
    assert L.bpe_window_holdback(b"\xf4\x90", 2, 0) == 0
    assert L.bpe_window_holdback(b"\xc1", 1, 0) == 0


@pytest.fixture()
def files(tmp_path):
    a = tmp_path / "a.txt"
    a.write_text("hello world")
    return tmp_path, a


def test_value_errors_without_a_device(files, monkeypatch):
    tmp, a = files
    tok = _tok()
    called = []
    monkeypatch.setattr(bpe_amd.Tokenizer, "_device", lambda self: called.append(1))
    out, idx = tmp / "o.bin", tmp / "o.idx"
    bad = [
        dict(dtype=np.int32),
        dict(dtype=np.uint8),
        dict(dtype="float32"),
        dict(window_bytes=65535),
        dict(window_bytes=0),
        dict(chars_per_piece=0),
        dict(separator="<|endoftext|>"),
        dict(index_path=idx),
        dict(separator="<|nope|>", index_path=idx),
        dict(separator=-1, index_path=idx),
        dict(separator=256, index_path=out),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            bpe_amd.encode_files(tok, [a], out, **kw)
    with pytest.raises(ValueError):
        bpe_amd.encode_files(tok, [a], a)
    with pytest.raises(ValueError):
        bpe_amd.encode_files(tok, [a], tmp / "sub" / ".." / "a.txt")
    with pytest.raises(ValueError):
        bpe_amd.encode_files(tok, [a], out, separator=256, index_path=a)
    link = tmp / "link.txt"
    link.symlink_to(a)
    with pytest.raises(ValueError):
        bpe_amd.encode_files(tok, [a], link)
    assert not called and not out.exists() and not idx.exists()
    assert a.read_text() == "hello world"


def test_missing_file_is_reported_before_the_device(files, monkeypatch):
    tmp, a = files
    called = []
    monkeypatch.setattr(bpe_amd.Tokenizer, "_device", lambda self: called.append(1))
    with pytest.raises(FileNotFoundError):
        bpe_amd.encode_files(_tok(), [a, tmp / "missing.txt"], tmp / "o.bin")
    assert not called and not (tmp / "o.bin").exists()


def test_helper_argument_checks():
    with pytest.raises(ValueError):
        bpe_amd.id_counts(np.zeros(4, dtype=np.uint16), 10)
    with pytest.raises(ValueError):
        bpe_amd.id_positions([1, 2, 3], 1)


def test_struct_layouts_match_the_header():
    # the sizes a C compiler gives the two structs of include/bpe355.h on LP64
    assert ctypes.sizeof(_lib.DatasetOpts) == 40
    assert ctypes.sizeof(_lib.DatasetStats) == 8 * 8 + 5 * 8
