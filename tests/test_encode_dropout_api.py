"""CPU-side checks of the encode-with-dropout boundary: include/bpe355.h declares the two entry
points, _lib.SYMBOLS binds them with the declared number of arguments, the library exports them,
and the Python methods validate p, seed and the document keys before the library is touched."""
import inspect
import pathlib
import re

import pytest

from bpe_amd import _lib

ROOT = pathlib.Path(__file__).resolve().parent.parent
NEW = {"bpe_tok_encode_dropout": 12, "bpe_tok_encode_dropout_device": 12}


def _declared_arity():
    text = (ROOT / "include" / "bpe355.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(bpe_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        args = args.strip()
        out[name] = 0 if args in ("", "void") else args.count(",") + 1
    return out


def test_header_declares_dropout_functions():
    arity = _declared_arity()
    assert {n: arity.get(n) for n in NEW} == NEW


def test_symbols_match_header_arity():
    sigs = {name: args for name, _res, args in _lib._SIGS}
    L = _lib.lib()
    for n, k in NEW.items():
        assert n in _lib.SYMBOLS and len(sigs[n]) == k and hasattr(L, n)
    assert L.bpe_abi_version() == 2   # additive: the ABI version stays


def test_python_signatures():
    import bpe_amd
    T = bpe_amd.Tokenizer
    P = inspect.Parameter
    assert list(inspect.signature(T.encode_dropout).parameters) == ["self", "text", "p", "seed", "doc_key"]
    assert inspect.signature(T.encode_dropout).parameters["doc_key"].default == 0
    for m in (T.encode_batch_dropout, T.encode_batch_dropout_np):
        p = inspect.signature(m).parameters
        assert list(p) == ["self", "texts", "p", "seed", "doc_base"] and p["doc_base"].default == 0
        assert p["p"].default is P.empty and p["seed"].default is P.empty
    p = inspect.signature(T.encode_batch_padded_dropout).parameters
    assert list(p) == ["self", "texts", "max_length", "pad_id", "p", "seed", "doc_base", "truncation", "padding_side",
                       "dtype"]
    assert p["max_length"].default is None and p["max_length"].kind is P.POSITIONAL_OR_KEYWORD
    for k in ("pad_id", "p", "seed", "doc_base", "truncation", "padding_side", "dtype"):
        assert p[k].kind is P.KEYWORD_ONLY
    assert p["pad_id"].default is P.empty and p["p"].default is P.empty and p["seed"].default is P.empty
    q = inspect.signature(T.encode_batch_padded).parameters
    assert all(p[k].default == q[k].default for k in ("truncation", "padding_side", "dtype"))


BAD = [   # (p, seed, key): one of them invalid
    (-0.01, 0, 0), (1.0000001, 0, 0), (float("nan"), 0, 0), (float("inf"), 0, 0), ("0.5", 0, 0), (None, 0, 0),
    (0.5j, 0, 0), (True, 0, 0),
    (0.5, -1, 0), (0.5, 2 ** 64, 0), (0.5, 1.0, 0), (0.5, "1", 0), (0.5, None, 0), (0.5, True, 0),
    (0.5, 0, -1), (0.5, 0, 2 ** 64), (0.5, 0, 0.0), (0.5, 0, None),
]


def test_bad_arguments_raise_before_the_library(monkeypatch):
    import bpe_amd
    tok = bpe_amd.Tokenizer({i: bytes([i]) for i in range(256)}, [], [])

    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(tok, "_device", boom)
    monkeypatch.setattr(_lib, "lib", boom)
    for p, seed, key in BAD:
        for call in (lambda: tok.encode_dropout("abc", p, seed, key),
                     lambda: tok.encode_batch_dropout(["abc"], p, seed, key),
                     lambda: tok.encode_batch_dropout_np(["abc"], p, seed, key),
                     lambda: tok.encode_batch_padded_dropout(["abc"], 4, pad_id=0, p=p, seed=seed, doc_base=key)):
            with pytest.raises(ValueError):
                call()
    # doc_base + len(texts) must stay below 2^64; the last key itself is fine for one document
    for call in (lambda: tok.encode_batch_dropout(["a", "b"], 0.5, 0, 2 ** 64 - 2),
                 lambda: tok.encode_batch_dropout_np(["a"] * 3, 0.5, 0, 2 ** 64 - 3),
                 lambda: tok.encode_dropout("a", 0.5, 0, 2 ** 64 - 1),
                 lambda: tok.encode_batch_padded_dropout(["a", "b"], 4, pad_id=0, p=0.5, seed=0, doc_base=2 ** 64 - 2)):
        with pytest.raises(ValueError, match="2\\^64"):
            call()
    for kw in ({"truncation": "middle"}, {"padding_side": "up"}, {"max_length": -1}):
        args = {"max_length": 4, "pad_id": 0, "p": 0.5, "seed": 1}
        args.update(kw)
        with pytest.raises(ValueError):
            tok.encode_batch_padded_dropout(["abc"], **args)


def test_valid_arguments_reach_the_library(monkeypatch):
    import bpe_amd
    tok = bpe_amd.Tokenizer({i: bytes([i]) for i in range(256)}, [], [])

    class Touched(Exception):
        pass

    def boom(*a, **k):
        raise Touched()
    monkeypatch.setattr(tok, "_device", boom)
    import numpy as np
    for p, seed, key in ((0, 0, 0), (1, 2 ** 64 - 1, 2 ** 64 - 2), (0.25, 7, 3), (np.float32(0.5), np.int64(3), np.uint64(9))):
        with pytest.raises(Touched):
            tok.encode_dropout("abc", p, seed, key)
        with pytest.raises(Touched):
            tok.encode_batch_dropout_np(["abc"], p, seed, key)


def test_thr_is_rounded_in_python():
    import bpe_amd
    f = bpe_amd.Tokenizer._dropout_args
    assert [f(p, 0, 0) for p in (0, 0.1, 0.5, 1.0, 1)] == [0, 1677722, 8388608, 16777216, 16777216]
