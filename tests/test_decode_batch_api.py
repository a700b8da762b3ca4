"""CPU-side checks of the batch-decode boundary: include/bpe355.h declares the three entry points,
_lib._SIGS binds them with the declared number of arguments, the library exports them, the five
Python methods exist, and without a GPU each raises what decode() raises (no CPU fallback)."""
import pathlib
import re

import pytest

from bpe_amd import _lib

ROOT = pathlib.Path(__file__).resolve().parent.parent
NEW = {"bpe_dec_decode_batch": 9, "bpe_dec_decode_batch_device": 11, "bpe_dec_decode_rows_device": 12}
METHODS = ("decode_batch", "decode_batch_bytes", "decode_batch_np", "decode_batch_padded", "decode_tokens")


def _declared_arity():
    text = (ROOT / "include" / "bpe355.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(bpe_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        args = args.strip()
        out[name] = 0 if args in ("", "void") else args.count(",") + 1
    return out


def test_header_declares_batch_decode_functions():
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


def test_python_methods_exist():
    import bpe_amd
    for m in METHODS:
        assert callable(getattr(bpe_amd.Tokenizer, m))


def test_decode_batch_needs_a_gpu():
    import numpy as np
    import torch
    import bpe_amd
    if _lib.lib().bpe_device_count() > 0:
        pytest.skip("a GPU is visible")
    tok = bpe_amd.Tokenizer({i: bytes([i]) for i in range(256)}, [], [])
    with pytest.raises(RuntimeError) as e_dec:
        tok.decode([1])
    ids, offs = np.array([1, 2, 3], dtype=np.uint32), np.array([0, 2, 3], dtype=np.int64)
    calls = [
        lambda: tok.decode_batch([[1, 2], [3]]), lambda: tok.decode_batch([]),
        lambda: tok.decode_batch_bytes([[1, 2], [3]]), lambda: tok.decode_batch_bytes([]),
        lambda: tok.decode_batch_np(ids, offs), lambda: tok.decode_batch_np(ids[:0], offs[:1]),
        lambda: tok.decode_batch_padded(torch.tensor([[1, 2], [3, 0]])),
        lambda: tok.decode_batch_padded(torch.zeros((0, 4), dtype=torch.int32)),
        lambda: tok.decode_tokens([1, 2, 3]), lambda: tok.decode_tokens([]),
    ]
    for call in calls:
        with pytest.raises(RuntimeError) as e:
            call()
        assert str(e.value) == str(e_dec.value)
