"""CPU-side checks of the batch-encode boundary: include/bpe355.h declares the three entry points,
_lib.SYMBOLS binds them with the declared number of arguments, the library exports them, and
without a GPU the Python methods raise what encode() raises (no CPU fallback)."""
import pathlib
import re

import pytest

from bpe_amd import _lib

ROOT = pathlib.Path(__file__).resolve().parent.parent
NEW = ["bpe_tok_encode_batch", "bpe_tok_encode_batch_device", "bpe_ids_pack_rows_device"]


def _declared_arity():
    text = (ROOT / "include" / "bpe355.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(bpe_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        args = args.strip()
        out[name] = 0 if args in ("", "void") else args.count(",") + 1
    return out


def test_header_declares_batch_functions():
    arity = _declared_arity()
    assert {n: arity.get(n) for n in NEW} == {"bpe_tok_encode_batch": 9, "bpe_tok_encode_batch_device": 9,
                                              "bpe_ids_pack_rows_device": 10}


def test_symbols_match_header_arity():
    arity = _declared_arity()
    sigs = {name: args for name, _res, args in _lib._SIGS}
    for n in NEW:
        assert n in _lib.SYMBOLS
        assert len(sigs[n]) == arity[n], n
    L = _lib.lib()
    for n in NEW:
        assert hasattr(L, n)
    assert L.bpe_abi_version() == 2


def test_python_methods_exist():
    import bpe_amd
    for m in ("encode_batch", "encode_batch_np", "encode_batch_padded"):
        assert callable(getattr(bpe_amd.Tokenizer, m))


def test_encode_batch_needs_a_gpu():
    import bpe_amd
    if _lib.lib().bpe_device_count() > 0:
        pytest.skip("a GPU is visible")
    tok = bpe_amd.Tokenizer({i: bytes([i]) for i in range(256)}, [], [])
    with pytest.raises(RuntimeError) as e_enc:
        tok.encode("abc")
    for call in (lambda: tok.encode_batch(["abc", "de"]), lambda: tok.encode_batch_np(["abc", "de"]),
                 lambda: tok.encode_batch([])):
        with pytest.raises(RuntimeError) as e:
            call()
        assert str(e.value) == str(e_enc.value)
    with pytest.raises(RuntimeError):
        tok.encode_batch_padded(["abc"], 4, pad_id=0)
