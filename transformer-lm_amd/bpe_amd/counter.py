"""WordCounter -- count pre-tokens over many inputs on the device, then train on the counts.

The reference's trainer sees its corpus only through {pre-token: count} (train.py:16-49), so a
counter fed shard by shard, or a file window by window, trains to exactly what train_bpe gives
on the same documents: many files, a corpus larger than HBM, pre-counted words, several vocab
sizes or special-token lists from one count.  Each add_* call is one document (its pre-tokens end
at its ends); special tokens only matter to counts() and train().
"""
from __future__ import annotations

import ctypes
import os
import struct
from typing import Iterable, List, Mapping

from . import _lib
from . import train as _train
from . import utf8 as _utf8

__all__ = ["WordCounter", "train_bpe_files", "train_bpe_word_counts"]


def _check(rc, what):
    if rc == _lib.BPE_E_ARG:
        msg = (_lib.lib().bpe_last_error() or b"").decode("utf-8", "replace")
        raise ValueError(f"libbpe355 {what} failed ({rc}): {msg}")
    _lib.check(rc, what)


class WordCounter:
    """A device-resident word table on the current GPU.  Not consumed by train(): add more and
    train again.  close() (or garbage collection) frees its device memory."""

    def __init__(self):
        self._h = None
        _lib.require_device()
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().bpe_counter_create(ctypes.byref(h)), "WordCounter()")
        self._h = h

    def _handle(self):
        if not self._h:
            raise ValueError("the WordCounter is closed")
        return self._h

    def _decode_as(self, errors: str, call, what: str, path=None):
        """Run one add call under the errors mode; a non-strict call leaves its report in
        bpe_amd.last_utf8_errors().  "strict" runs the call exactly as it always did."""
        mode = _utf8.mode_of(errors)
        if mode == 0:
            _check(call(), what)
            return self
        L = _lib.lib()
        h = self._handle()
        _check(L.bpe_counter_set_errors(h, mode), what)
        try:
            _check(call(), what)
            st = _lib.Utf8Stats()
            _check(L.bpe_counter_utf8_report(h, ctypes.byref(st)), what)
        finally:
            L.bpe_counter_set_errors(h, 0)
        d = _utf8.stats_dict(st)
        _utf8.note(errors, d["n_units"], d["n_bytes"], (path, d["first"]) if d["first"] is not None else None)
        return self

    def add_file(self, path: str | os.PathLike, window_bytes: int | None = None, errors: str = "strict"):
        """The file as train_bpe reads it, counted in windows of about window_bytes (None: the
        library's default, 8 GiB) so that only one window is in device memory at a time.  After
        an error (FileNotFoundError / OSError, UnicodeDecodeError) the counter is unchanged.
        errors: "strict", or "replace" / "ignore" as open(path, encoding="utf-8", errors=...)
        reads the file: a window with ill-formed UTF-8 is repaired on the device and counted."""
        _utf8.mode_of(errors)
        return self._decode_as(errors, lambda: _lib.lib().bpe_counter_add_file(
            self._handle(), os.fsencode(os.fspath(path)), int(window_bytes or 0)),
            f"WordCounter.add_file({os.fspath(path)!r})", os.fspath(path))

    def add_bytes(self, data: bytes, errors: str = "strict"):
        """Raw file bytes (decoded exactly like the file would be): one document."""
        _utf8.mode_of(errors)
        data = bytes(data)
        return self._decode_as(errors, lambda: _lib.lib().bpe_counter_add_buffer(self._handle(), data, len(data)),
                               "WordCounter.add_bytes")

    def add_text(self, text: str):
        return self.add_bytes(text.encode("utf-8"))

    def add_tensor(self, t, errors: str = "strict"):
        """A contiguous uint8 tensor on the counter's GPU holding raw file bytes; it is not modified."""
        _utf8.mode_of(errors)
        import torch
        if t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous():
            raise ValueError("add_tensor needs a contiguous uint8 cuda tensor")
        stream = torch.cuda.current_stream(t.device).cuda_stream
        return self._decode_as(errors, lambda: _lib.lib().bpe_counter_add_device(
            self._handle(), ctypes.c_void_p(t.data_ptr()), t.numel(), ctypes.c_void_p(stream or None)),
            "WordCounter.add_tensor")

    def add_counts(self, counts: Mapping):
        """Pre-counted words {str | bytes: int}; words under 2 bytes carry no pair and are dropped."""
        parts = []
        for w, c in counts.items():
            b = w.encode("utf-8") if isinstance(w, str) else bytes(w)
            parts.append(struct.pack("<I", len(b)) + b + struct.pack("<Q", int(c)))
        blob = b"".join(parts)
        _check(_lib.lib().bpe_counter_add_words(self._handle(), blob, len(blob)), "WordCounter.add_counts")
        return self

    def add_words_blob(self, blob: bytes):
        """(u32 len, bytes, u64 count) records, as bpe_counter_words returns them."""
        _check(_lib.lib().bpe_counter_add_words(self._handle(), blob, len(blob)), "WordCounter.add_words_blob")
        return self

    def absorb(self, other: "WordCounter"):
        """Add everything `other` holds; `other` is unchanged."""
        _check(_lib.lib().bpe_counter_absorb(self._handle(), other._handle()), "WordCounter.absorb")
        return self

    def counts(self, special_tokens: Iterable[str] = ()) -> dict:
        """{word bytes: count} of the multi-byte pre-tokens not equal to a special token."""
        L = _lib.lib()
        arr, n, _keep = _lib.c_strings(special_tokens)
        blob, nb = ctypes.c_void_p(), ctypes.c_size_t(0)
        _check(L.bpe_counter_words(self._handle(), arr, n, ctypes.byref(blob), ctypes.byref(nb)), "WordCounter.counts")
        try:
            data = ctypes.string_at(blob, nb.value) if nb.value else b""
        finally:
            L.bpe_blob_free(blob)
        out, off = {}, 0
        while off < len(data):
            ln = struct.unpack_from("<I", data, off)[0]
            out[data[off + 4:off + 4 + ln]] = struct.unpack_from("<Q", data, off + 4 + ln)[0]
            off += 12 + ln
        return out

    def info(self) -> dict:
        i = _lib.CounterInfo()
        _check(_lib.lib().bpe_counter_info(self._handle(), ctypes.byref(i)), "WordCounter.info")
        return i.as_dict()

    def train(self, vocab_size: int, special_tokens: List[str] = []):
        """(vocab, merges) as train_bpe returns them, from the counted words; sets last_train_stats()."""
        arr, n, _keep = _lib.c_strings(special_tokens)
        res = ctypes.c_void_p()
        rc = _lib.lib().bpe_counter_train(self._handle(), int(vocab_size), arr, n, ctypes.byref(res))
        _check(rc, "WordCounter.train")
        vocab, merges, stats = _lib.take_result(res)
        _train._last_stats = stats
        return vocab, merges

    def clear(self):
        _lib.lib().bpe_counter_clear(self._handle())

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            _lib.lib().bpe_counter_free(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _train_and_release(counter, fill, vocab_size, special_tokens):
    try:
        fill(counter)
        return counter.train(vocab_size, special_tokens)
    finally:
        counter.close()
        try:
            _train.release_device_memory(-1)
        except Exception:
            pass


def train_bpe_files(paths, vocab_size: int, special_tokens: List[str] = [], window_bytes: int | None = None,
                    errors: str = "strict"):
    """train_bpe over several files, each one document, none of them held in device memory beyond
    one window of window_bytes: what the reference gives on a corpus whose documents they are.
    errors: as WordCounter.add_file; last_utf8_errors() then sums over the files."""
    if _utf8.mode_of(errors) == 0:
        def fill(c):
            for p in paths:
                c.add_file(p, window_bytes)
    else:
        def fill(c):
            n_units = n_bytes = 0
            first = None
            for p in paths:
                c.add_file(p, window_bytes, errors=errors)
                r = _utf8.last_utf8_errors()
                n_units += r["n_units"]
                n_bytes += r["n_bytes"]
                first = first or r["first"]
            _utf8.note(errors, n_units, n_bytes, first)
    return _train_and_release(WordCounter(), fill, vocab_size, special_tokens)


def train_bpe_word_counts(counts: Mapping, vocab_size: int, special_tokens: List[str] = []):
    """train_bpe from pre-counted words {str | bytes: int} (the reference's merge loop on them)."""
    return _train_and_release(WordCounter(), lambda c: c.add_counts(counts), vocab_size, special_tokens)
