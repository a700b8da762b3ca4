"""CPU-side checks of the word-counter boundary: include/bpe355.h declares the bpe_counter_*
entry points, _lib._SIGS binds them with the declared number of arguments, the library exports
them, the Python names exist, and without a GPU each raises RuntimeError (no CPU fallback)."""
import ctypes
import pathlib
import re

import pytest

from bpe_amd import _lib

ROOT = pathlib.Path(__file__).resolve().parent.parent
NEW = {"bpe_counter_create": 1, "bpe_counter_add_file": 3, "bpe_counter_add_buffer": 3,
       "bpe_counter_add_device": 4, "bpe_counter_add_words": 3, "bpe_counter_absorb": 2,
       "bpe_counter_words": 5, "bpe_counter_train": 5, "bpe_counter_info": 2,
       "bpe_counter_clear": 1, "bpe_counter_free": 1}
METHODS = ("add_file", "add_bytes", "add_text", "add_tensor", "add_counts", "absorb", "counts", "info",
           "clear", "close", "train")


def _declared_arity():
    text = (ROOT / "include" / "bpe355.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(bpe_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        args = args.strip()
        out[name] = 0 if args in ("", "void") else args.count(",") + 1
    return out


def test_header_declares_counter_functions():
    arity = _declared_arity()
    assert {n: arity.get(n) for n in NEW} == NEW


def test_symbols_match_header_arity():
    arity = _declared_arity()
    sigs = {name: args for name, _res, args in _lib._SIGS}
    for n, k in NEW.items():
        assert n in _lib.SYMBOLS
        assert len(sigs[n]) == arity[n] == k, n
    L = _lib.lib()
    for n in NEW:
        assert hasattr(L, n)
    assert L.bpe_abi_version() == 2


def test_info_struct_matches_header():
    text = (ROOT / "include" / "bpe355.h").read_text()
    body = re.search(r"typedef struct \{([^}]*)\} bpe_counter_info_t;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(uint64_t|double)\s+([a-z_]+)\s*;", body)
    assert [f for _t, f in fields] == [f for f, _t in _lib.CounterInfo._fields_]
    for (t, _f), (_g, ct) in zip(fields, _lib.CounterInfo._fields_):
        assert ct is {"uint64_t": ctypes.c_uint64, "double": ctypes.c_double}[t]


def test_python_names_exist():
    import bpe_amd
    for m in METHODS:
        assert callable(getattr(bpe_amd.WordCounter, m))
    assert callable(bpe_amd.train_bpe_files) and callable(bpe_amd.train_bpe_word_counts)


def test_counter_needs_a_gpu(tmp_path):
    import bpe_amd
    if _lib.lib().bpe_device_count() > 0:
        pytest.skip("a GPU is visible")
    p = tmp_path / "c.txt"
    p.write_bytes(b"abc abc")
    calls = [
        lambda: bpe_amd.WordCounter(),
        lambda: bpe_amd.train_bpe_files([p], 300, []),
        lambda: bpe_amd.train_bpe_files([], 300, []),
        lambda: bpe_amd.train_bpe_word_counts({b" abc": 2}, 300, []),
    ]
    for call in calls:
        with pytest.raises(RuntimeError):
            call()
