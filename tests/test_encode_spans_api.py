"""CPU-side checks of the encode-with-offsets boundary: include/bpe355.h declares the two entry
points, _lib.SYMBOLS binds them with the declared number of arguments, the library exports them,
the Python methods validate `unit` before the library is touched, and without a GPU they raise
what encode() raises (no CPU fallback)."""
import inspect
import pathlib
import re

import pytest

from bpe_amd import _lib

ROOT = pathlib.Path(__file__).resolve().parent.parent
NEW = {"bpe_tok_encode_spans": 12, "bpe_tok_encode_spans_device": 11}
METHODS = ("encode_with_offsets", "encode_batch_offsets", "encode_batch_offsets_np", "encode_batch_padded_offsets")


def _declared_arity():
    text = (ROOT / "include" / "bpe355.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(bpe_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        args = args.strip()
        out[name] = 0 if args in ("", "void") else args.count(",") + 1
    return out


def test_header_declares_span_functions():
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
    for m in METHODS:
        p = inspect.signature(getattr(bpe_amd.Tokenizer, m)).parameters
        assert p["unit"].default == "char", m
    p = inspect.signature(bpe_amd.Tokenizer.encode_batch_padded_offsets).parameters
    q = inspect.signature(bpe_amd.Tokenizer.encode_batch_padded).parameters
    assert list(p)[:-1] == list(q) and all(p[k].default == q[k].default and p[k].kind == q[k].kind for k in q)
    assert p["unit"].kind is inspect.Parameter.KEYWORD_ONLY


def test_unknown_unit_raises_before_the_library(monkeypatch):
    import bpe_amd
    tok = bpe_amd.Tokenizer({i: bytes([i]) for i in range(256)}, [], [])

    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(tok, "_device", boom)
    monkeypatch.setattr(_lib, "lib", boom)
    for unit in ("bogus", "bytes", "", None, 0):
        for call in (lambda: tok.encode_with_offsets("abc", unit), lambda: tok.encode_batch_offsets(["abc"], unit),
                     lambda: tok.encode_batch_offsets_np(["abc"], unit),
                     lambda: tok.encode_batch_padded_offsets(["abc"], 4, pad_id=0, unit=unit)):
            with pytest.raises(ValueError, match="unit"):
                call()


def test_padded_argument_checks_come_first():
    import bpe_amd
    tok = bpe_amd.Tokenizer({i: bytes([i]) for i in range(256)}, [], [])
    pytest.importorskip("torch")
    for kw in ({"truncation": "middle"}, {"padding_side": "up"}, {"dtype": float}, {"max_length": -1}):
        args = {"max_length": 4, "pad_id": 0}
        args.update(kw)
        with pytest.raises(ValueError):
            tok.encode_batch_padded_offsets(["abc"], **args)


def test_span_calls_need_a_gpu():
    import bpe_amd
    if _lib.lib().bpe_device_count() > 0:
        pytest.skip("a GPU is visible")
    tok = bpe_amd.Tokenizer({i: bytes([i]) for i in range(256)}, [], [])
    with pytest.raises(RuntimeError) as e_enc:
        tok.encode("abc")
    for call in (lambda: tok.encode_with_offsets("abc"), lambda: tok.encode_batch_offsets(["abc", "de"], "byte"),
                 lambda: tok.encode_batch_offsets_np(["abc", "de"])):
        with pytest.raises(RuntimeError) as e:
            call()
        assert str(e.value) == str(e_enc.value)
    with pytest.raises(RuntimeError):
        tok.encode_batch_padded_offsets(["abc"], 4, pad_id=0)
