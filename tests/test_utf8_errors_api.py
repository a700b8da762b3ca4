"""The errors= keyword without a device: a value other than "strict", "replace", "ignore" raises
ValueError from every entry point before the device is touched, and a non-strict mode cannot be
combined with comm or split_file.  The new C symbols are declared, bound and exported."""
import pathlib
import re

import pytest

import bpe_amd
from bpe_amd import _lib
from bpe_amd import encode as enc

ROOT = pathlib.Path(__file__).resolve().parent.parent
NEW = {"bpe_utf8_repair_device": 8, "bpe_utf8_repair_geometry": 2, "bpe_text_prepare_device_ex": 8,
       "bpe_counter_set_errors": 2, "bpe_counter_utf8_report": 2, "bpe_tok_set_errors": 2,
       "bpe_tok_utf8_report": 5}
BAD = ("surrogateescape", "", "Replace", None, 1)


def _tok():
    return bpe_amd.Tokenizer({i: bytes([i]) for i in range(256)}, [], [])


def _counter():
    c = object.__new__(bpe_amd.WordCounter)   # no device: the constructor would need one
    c._h = None
    return c


def _calls(errors, tmp_path):
    p = tmp_path / "t.txt"
    p.write_bytes(b"abc abc")
    out = tmp_path / "o.bin"
    return {
        "train_bpe": lambda: bpe_amd.train_bpe(p, 300, [], errors=errors),
        "train_bpe_bytes": lambda: bpe_amd.train_bpe_bytes(b"abc", 300, [], errors=errors),
        "train_bpe_files": lambda: bpe_amd.train_bpe_files([p], 300, [], errors=errors),
        "add_file": lambda: _counter().add_file(p, errors=errors),
        "add_bytes": lambda: _counter().add_bytes(b"abc", errors=errors),
        "add_tensor": lambda: _counter().add_tensor(object(), errors=errors),
        "encode_file": lambda: enc.encode_file(_tok(), p, errors=errors),
        "encode_bytes_u16": lambda: enc.encode_bytes_u16(_tok(), b"abc", errors=errors),
        "encode_device_u16": lambda: enc.encode_device_u16(_tok(), object(), errors=errors),
        "encode_files": lambda: bpe_amd.encode_files(_tok(), [p], out, errors=errors),
        "repair_utf8": lambda: bpe_amd.repair_utf8(b"abc", errors=errors),
    }


@pytest.mark.parametrize("bad", BAD, ids=repr)
def test_bad_errors_value_is_a_value_error_everywhere(bad, tmp_path):
    for name, call in _calls(bad, tmp_path).items():
        with pytest.raises(ValueError, match="errors"):
            call()
    assert not (tmp_path / "o.bin").exists()


def test_repair_utf8_is_not_strict():
    with pytest.raises(ValueError):
        bpe_amd.repair_utf8(b"abc", errors="strict")


@pytest.mark.parametrize("mode", ["replace", "ignore"])
def test_non_strict_refuses_comm_and_split_file(mode, tmp_path):
    p = tmp_path / "t.txt"
    p.write_bytes(b"abc abc")
    comm = object()   # never looked at: the combination is refused first
    with pytest.raises(ValueError, match="comm"):
        bpe_amd.train_bpe(p, 300, [], comm=comm, errors=mode)
    with pytest.raises(ValueError, match="split_file"):
        bpe_amd.train_bpe(p, 300, [], split_file=True, errors=mode)
    with pytest.raises(ValueError, match="comm"):
        bpe_amd.train_bpe_bytes(b"abc", 300, [], comm=comm, errors=mode)


def test_new_symbols_declared_bound_and_exported():
    text = (ROOT / "include" / "bpe355.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    arity = {name: args.count(",") + 1 for name, args in re.findall(r"\b(bpe_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text)}
    sigs = {name: args for name, _res, args in _lib._SIGS}
    L = _lib.lib()
    for n, k in NEW.items():
        assert arity.get(n) == k == len(sigs[n]), n
        assert hasattr(L, n)
    assert L.bpe_abi_version() == 2
    unit, tile = bpe_amd.utf8.repair_geometry()   # needs no device
    assert unit == 16 and tile % (64 * unit) == 0


def test_last_utf8_errors_is_a_copy():
    r = bpe_amd.last_utf8_errors()
    r["x"] = 1
    assert "x" not in bpe_amd.last_utf8_errors()
