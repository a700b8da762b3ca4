"""Tokenizer -- drop-in for reference models/tokenizer/tokenizer.py:11-167.

Construction rules, special-token handling and the encode result follow the reference
exactly; encode() runs on the GPU through libbpe355 (segmentation on special tokens,
GPT-2 pre-tokenization, per-word rank-ordered merges, id lookup).  decode(), save() and
from_files() are host-side byte/pickle plumbing, as in the reference.
"""
from __future__ import annotations

import ctypes
import itertools
import os
import pickle
from typing import Iterable, Iterator, List, Tuple

from . import _lib
from .train import train_bpe


class Tokenizer:
    def __init__(self, vocab: dict[int, bytes], merges: List[Tuple[bytes, bytes]],
                 special_tokens: List[str] | None = []):
        # tokenizer.py:18-38, including its bookkeeping quirks: vocab_inv keeps the LAST id of
        # a repeated byte string, and a missing special is appended as
        # self.vocab[bytes] = len(self.vocab) with vocab_inv[bytes] = len(self.vocab) - 1.
        self.vocab = vocab
        self.vocab_inv = {v: k for k, v in vocab.items()}
        self.merges = merges
        seen = set()
        specials = []
        for t in special_tokens or []:
            if t not in seen:
                seen.add(t)
                specials.append(t)
        # longest first; equal lengths keep first-occurrence order (the reference uses set
        # iteration order there, which only matters for the ids of equal-length missing specials)
        specials.sort(key=len, reverse=True)
        self.special_tokens = specials
        for token in self.special_tokens:
            b = token.encode("utf-8")
            if b not in self.vocab_inv:
                self.vocab[b] = len(self.vocab)
                self.vocab_inv[b] = len(self.vocab) - 1
        self._handle = None
        self._dec = None

    # ------------------------------------------------------------------ constructors
    @classmethod
    def train_from_file(cls, filepath: str, vocab_size: int, special_tokens: List[str]):
        vocab, merges = train_bpe(filepath, vocab_size, special_tokens)
        return cls(vocab, merges, special_tokens)

    @classmethod
    def fit(cls, input_path: str, vocab_size: int, special_tokens: List[str]):
        vocab, merges = train_bpe(input_path, vocab_size, special_tokens)
        return cls(vocab, merges, special_tokens)

    @classmethod
    def from_files(cls, vocab_filepath: str, merges_filepath: str,
                   special_tokens: List[str] = []) -> "Tokenizer":
        # files written by Tokenizer.save (the caller's own artifacts), as in tokenizer.py:50-61
        with open(vocab_filepath, "rb") as f:
            vocab = pickle.load(f)
        with open(merges_filepath, "rb") as f:
            merges = pickle.load(f)
        return cls(vocab, merges, special_tokens=special_tokens)

    @classmethod
    def from_gpt2_files(cls, vocab_json: str, merges_txt: str,
                        special_tokens: List[str] | None = None) -> "Tokenizer":
        """GPT-2 vocab.json / merges.txt (formats.py), as the reference's tests load them."""
        from .formats import load_gpt2
        vocab, merges = load_gpt2(vocab_json, merges_txt, special_tokens)
        return cls(vocab, merges, special_tokens)

    def save_gpt2(self, vocab_json: str, merges_txt: str) -> None:
        from .formats import save_gpt2
        save_gpt2({i: b for i, b in self.vocab.items() if isinstance(i, int)}, self.merges,
                  vocab_json, merges_txt)

    # ------------------------------------------------------------------ device handle
    def _device(self):
        if self._handle is None:
            L = _lib.lib()
            # bytes -> int entries only: after save()/from_files() a missing special added by
            # the reference quirk (self.vocab[b] = len(vocab), tokenizer.py:35-38) comes back as
            # an int -> bytes entry of vocab_inv, which the reference's encode never consults
            inv = [(i, b) for b, i in self.vocab_inv.items()
                   if isinstance(b, (bytes, bytearray)) and isinstance(i, int)]
            vb = _lib.vocab_blob(dict(inv) if len({i for i, _ in inv}) == len(inv) else {})
            if len({i for i, _ in inv}) != len(inv):
                # several byte strings share an id: pass the pairs as they are
                import struct
                vb = struct.pack("<I", len(inv)) + b"".join(
                    struct.pack("<qI", int(i), len(b)) + bytes(b) for i, b in inv)
            mb = _lib.merges_blob(self.merges)
            arr, n, _keep = _lib.c_strings(self.special_tokens)
            h = ctypes.c_void_p()
            _lib.check(L.bpe_tok_create(vb, len(vb), mb, len(mb), arr, n, ctypes.byref(h)),
                       "Tokenizer")
            self._handle = h
        return self._handle

    def __del__(self):
        h = getattr(self, "_handle", None)
        d = getattr(self, "_dec", None)
        if _lib._lib is not None:
            try:
                if h is not None:
                    _lib._lib.bpe_tok_free(h)
                if d is not None:
                    _lib._lib.bpe_dec_free(d)
            except Exception:  # noqa: BLE001
                pass

    def release_device_buffers(self) -> None:
        """Free the device memory the encoder keeps between calls (its per-call arrays and the
        bulk encoder's text and uint16 ids, about 3 bytes per input byte); the tables stay."""
        if self._handle is not None:
            _lib.check(_lib.lib().bpe_tok_release_buffers(self._handle), "release")

    # ------------------------------------------------------------------ encode / decode
    def encode(self, text: str) -> List[int]:
        """tokenizer.py:111-138 on the GPU."""
        data = text.encode("utf-8")
        h = self._device()
        cap = max(1, len(data))
        out = (ctypes.c_uint32 * cap)()
        n_out = ctypes.c_size_t(0)
        from .train import num_gpus
        g = num_gpus()
        if g == 1:
            rc = _lib.lib().bpe_tok_encode(h, data, len(data), out, cap, ctypes.byref(n_out))
        else:   # one process, several devices (bpe_amd.set_num_gpus / BPE355_GPUS)
            rc = _lib.lib().bpe_tok_encode_gpus(h, data, len(data), out, cap, ctypes.byref(n_out), g)
        _lib.check(rc, "encode")
        return list(out[: n_out.value])

    # ------------------------------------------------------------------ batch encode
    # encode(t) for every t of a list in one launch sequence: the texts are joined, the library
    # encodes the join with a cut at every document start (bpe_tok_encode_batch: each document is
    # segmented and pre-tokenized on its own, so a seam never merges trailing whitespace, a
    # contraction or the halves of a special token) and reports where each document's ids begin.
    # These methods run on the current device whatever set_num_gpus / BPE355_GPUS says: spreading
    # the documents of one batch over devices is left to the caller.
    @staticmethod
    def _join(texts):
        import numpy as np
        datas = [t.encode("utf-8") for t in texts]
        starts = np.zeros(len(datas) + 1, dtype=np.uint64)
        if datas:
            np.cumsum(np.fromiter(map(len, datas), dtype=np.uint64, count=len(datas)), out=starts[1:])
        return b"".join(datas), starts

    def encode_batch_np(self, texts: List[str]):
        """-> (ids np.uint32 [total], offsets np.int64 [len(texts) + 1]): encode(texts[i]) is
        ids[offsets[i]:offsets[i + 1]].  One UTF-8 join, one library call, one copy back; on the
        current device (set_num_gpus does not apply)."""
        import numpy as np
        texts = list(texts)
        h = self._device()
        data, starts = self._join(texts)
        n, nd = len(data), len(texts)
        ids = np.empty(max(n, 1), dtype=np.uint32)
        offsets = np.zeros(nd + 1, dtype=np.uint64)
        n_out = ctypes.c_size_t(0)
        if nd:
            rc = _lib.lib().bpe_tok_encode_batch(h, data, n, starts.ctypes.data, nd, ids.ctypes.data, ids.size,
                                                 ctypes.byref(n_out), offsets.ctypes.data)
            _lib.check(rc, "encode_batch")
        return ids[:n_out.value].copy(), offsets.astype(np.int64)

    def encode_batch(self, texts: List[str]) -> List[List[int]]:
        """[encode(t) for t in texts] in one library call (see encode_batch_np); on the current
        device (set_num_gpus does not apply)."""
        ids, offsets = self.encode_batch_np(texts)
        flat, off = ids.tolist(), offsets.tolist()
        return [flat[a:b] for a, b in zip(off, off[1:])]

    def encode_batch_padded(self, texts: List[str], max_length: int | None = None, *, pad_id: int,
                            truncation: str = "right", padding_side: str = "right", dtype=None):
        """-> (tensor [len(texts), T] of dtype (torch.int64, or torch.int32) on the current device,
        int32 lengths [len(texts)]).  T is max_length, or the longest row when it is None.  A row
        longer than T loses ids on the `truncation` side ("right": the first T are kept, "left":
        the last T); a shorter one is filled with pad_id on `padding_side`.  lengths[i] =
        min(len(encode(texts[i])), T).  With torch.int32 a kept id of 2^31 or more raises RuntimeError
        (BPE_E_LIMIT, naming the id) instead of wrapping.  The text goes to the device once, the ids never leave it
        (bpe_tok_encode_batch_device, then bpe_ids_pack_rows_device); on the current device
        (set_num_gpus does not apply)."""
        import torch
        dtype = torch.int64 if dtype is None else dtype
        if truncation not in ("right", "left") or padding_side not in ("right", "left"):
            raise ValueError("truncation and padding_side are 'right' or 'left'")
        if dtype not in (torch.int32, torch.int64):
            raise ValueError("dtype is torch.int32 or torch.int64")
        if max_length is not None and max_length < 0:
            raise ValueError("max_length is negative")
        texts = list(texts)
        h = self._device()
        L = _lib.lib()
        data, starts = self._join(texts)
        n, nd = len(data), len(texts)
        dev = torch.device("cuda", torch.cuda.current_device())
        lengths = torch.zeros(nd, dtype=torch.int32, device=dev)
        if nd == 0:
            return torch.empty((0, max_length or 0), dtype=dtype, device=dev), lengths
        stream = torch.cuda.current_stream()
        sp = ctypes.c_void_p(stream.cuda_stream)
        d_ids = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        d_off = torch.zeros(nd + 1, dtype=torch.int64, device=dev)
        if n:
            d_text = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
            stream.synchronize()
            n_out = ctypes.c_size_t(0)
            _lib.check(L.bpe_tok_encode_batch_device(h, ctypes.c_void_p(d_text.data_ptr()), n, starts.ctypes.data, nd,
                                                     ctypes.c_void_p(d_ids.data_ptr()), ctypes.byref(n_out),
                                                     ctypes.c_void_p(d_off.data_ptr()), sp), "encode_batch")
        T = int((d_off[1:] - d_off[:-1]).max()) if max_length is None else int(max_length)
        out = torch.empty((nd, T), dtype=dtype, device=dev)
        flags = (1 if truncation == "left" else 0) | (2 if padding_side == "left" else 0)
        stream.synchronize()
        _lib.check(L.bpe_ids_pack_rows_device(ctypes.c_void_p(d_ids.data_ptr()), ctypes.c_void_p(d_off.data_ptr()), nd,
                                              T, int(pad_id), flags, 4 if dtype == torch.int32 else 8,
                                              ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(lengths.data_ptr()),
                                              sp), "pack rows")
        return out, lengths

    # ------------------------------------------------------------------ encode with offsets
    # The batch encode, and for every id the half-open span of its document's text that produced
    # it (bpe_tok_encode_spans): unit="byte" indexes text.encode("utf-8"), unit="char" (the
    # default: callers hold str) indexes the str.  A leading space belongs to its token; a special
    # token's span is the special; a pre-token equal to a special yields no id, so the next span
    # starts past it.  A byte-level token that begins or ends inside a character covers that
    # character, so text[s:e].encode() always contains the token's bytes.  The ids are those of
    # encode() / encode_batch().  A vocab in which one id names byte strings of different lengths
    # has no per-id length: ValueError.  On the current device, like the batch encode.
    _UNITS = {"byte": 0, "char": 1}

    @classmethod
    def _unit(cls, unit) -> int:
        if not isinstance(unit, str) or unit not in cls._UNITS:
            raise ValueError("unit is 'byte' or 'char'")
        return cls._UNITS[unit]

    @staticmethod
    def _span_status(rc: int, what: str) -> None:
        if rc == _lib.BPE_E_ARG:
            raise ValueError((_lib.lib().bpe_last_error() or b"").decode("utf-8", "replace"))
        _lib.check(rc, what)

    def encode_batch_offsets_np(self, texts: List[str], unit: str = "char"):
        """-> (ids np.uint32 [N], id_offsets np.int64 [len(texts) + 1], spans np.int64 [N, 2]):
        document i's ids are ids[id_offsets[i]:id_offsets[i + 1]] and id j came from
        texts[i][spans[j, 0]:spans[j, 1]] (unit="byte": from those bytes of its UTF-8).  One join,
        one library call."""
        import numpy as np
        u = self._unit(unit)
        texts = list(texts)
        h = self._device()
        data, starts = self._join(texts)
        n, nd = len(data), len(texts)
        ids = np.empty(max(n, 1), dtype=np.uint32)
        spans = np.empty((max(n, 1), 2), dtype=np.uint32)
        offsets = np.zeros(nd + 1, dtype=np.uint64)
        n_out = ctypes.c_size_t(0)
        if nd:
            rc = _lib.lib().bpe_tok_encode_spans(h, data, n, starts.ctypes.data, nd, u, ids.ctypes.data, ids.size,
                                                 ctypes.byref(n_out), offsets.ctypes.data, spans.ctypes.data,
                                                 spans.shape[0])
            self._span_status(rc, "encode_spans")
        m = n_out.value
        return ids[:m].copy(), offsets.astype(np.int64), spans[:m].astype(np.int64)

    def encode_batch_offsets(self, texts: List[str], unit: str = "char"):
        """-> [(encode(t), [(start, end), ...]) for t in texts] in one library call."""
        ids, offsets, spans = self.encode_batch_offsets_np(texts, unit)
        flat, off = ids.tolist(), offsets.tolist()
        sp = [tuple(x) for x in spans.tolist()]
        return [(flat[a:b], sp[a:b]) for a, b in zip(off, off[1:])]

    def encode_with_offsets(self, text: str, unit: str = "char") -> Tuple[List[int], List[Tuple[int, int]]]:
        """-> (encode(text), [(start, end) of every id])."""
        ids, _, spans = self.encode_batch_offsets_np([text], unit)
        return ids.tolist(), [tuple(x) for x in spans.tolist()]

    def encode_batch_padded_offsets(self, texts: List[str], max_length: int | None = None, *, pad_id: int,
                                    truncation: str = "right", padding_side: str = "right", dtype=None,
                                    unit: str = "char"):
        """encode_batch_padded with the spans: -> (ids [B, T], int32 lengths [B], spans [B, T, 2]
        torch.int64), all on the current device; the ids and lengths are encode_batch_padded's, a
        kept id's span stands at its position and a padding position holds (0, 0).  The ids and the
        spans never leave the device (bpe_tok_encode_spans_device, then bpe_ids_pack_rows_device
        for the ids and for each span column)."""
        import torch
        u = self._unit(unit)
        dtype = torch.int64 if dtype is None else dtype
        if truncation not in ("right", "left") or padding_side not in ("right", "left"):
            raise ValueError("truncation and padding_side are 'right' or 'left'")
        if dtype not in (torch.int32, torch.int64):
            raise ValueError("dtype is torch.int32 or torch.int64")
        if max_length is not None and max_length < 0:
            raise ValueError("max_length is negative")
        texts = list(texts)
        h = self._device()
        L = _lib.lib()
        data, starts = self._join(texts)
        n, nd = len(data), len(texts)
        dev = torch.device("cuda", torch.cuda.current_device())
        lengths = torch.zeros(nd, dtype=torch.int32, device=dev)
        if nd == 0:
            T0 = max_length or 0
            return (torch.empty((0, T0), dtype=dtype, device=dev), lengths,
                    torch.empty((0, T0, 2), dtype=torch.int64, device=dev))
        stream = torch.cuda.current_stream()
        sp = ctypes.c_void_p(stream.cuda_stream)
        d_ids = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        d_spans = torch.zeros((max(n, 1), 2), dtype=torch.int32, device=dev)
        d_off = torch.zeros(nd + 1, dtype=torch.int64, device=dev)
        if n:
            d_text = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
            stream.synchronize()
            n_out = ctypes.c_size_t(0)
            self._span_status(L.bpe_tok_encode_spans_device(
                h, ctypes.c_void_p(d_text.data_ptr()), n, starts.ctypes.data, nd, u, ctypes.c_void_p(d_ids.data_ptr()),
                ctypes.byref(n_out), ctypes.c_void_p(d_off.data_ptr()), ctypes.c_void_p(d_spans.data_ptr()), sp),
                "encode_spans")
        T = int((d_off[1:] - d_off[:-1]).max()) if max_length is None else int(max_length)
        out = torch.empty((nd, T), dtype=dtype, device=dev)
        flags = (1 if truncation == "left" else 0) | (2 if padding_side == "left" else 0)
        cols = [d_spans[:, k].contiguous() for k in (0, 1)]   # (uint32 values in int32 storage)
        packed = [torch.empty((nd, T), dtype=torch.int64, device=dev) for _ in cols]
        scratch = torch.empty(nd, dtype=torch.int32, device=dev)
        stream.synchronize()
        _lib.check(L.bpe_ids_pack_rows_device(ctypes.c_void_p(d_ids.data_ptr()), ctypes.c_void_p(d_off.data_ptr()), nd,
                                              T, int(pad_id), flags, 4 if dtype == torch.int32 else 8,
                                              ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(lengths.data_ptr()),
                                              sp), "pack rows")
        for col, dst in zip(cols, packed):
            _lib.check(L.bpe_ids_pack_rows_device(ctypes.c_void_p(col.data_ptr()), ctypes.c_void_p(d_off.data_ptr()), nd,
                                                  T, 0, flags, 8, ctypes.c_void_p(dst.data_ptr()),
                                                  ctypes.c_void_p(scratch.data_ptr()), sp), "pack rows")
        return out, lengths, torch.stack(packed, dim=-1)

    # ------------------------------------------------------------------ encode with BPE-dropout
    # The batch encode with subword regularisation (Provilkov et al., 2020; HF tokenizers'
    # BPE(dropout=p)): while a pre-token is merged, every candidate merge is skipped with
    # probability p.  The draws are counter-based (bpe_tok_encode_dropout in include/bpe355.h), so
    # the ids of a document depend only on (seed, doc_key, text) -- not on the batch it is in: row
    # i of a batch draws with doc_key = doc_base + i.  p = 0 is encode(); p = 1 gives every byte
    # its own id.  Specials, the pre-tokenization and KeyError are encode()'s.  On the current
    # device, like the batch encode.
    _U64 = 1 << 64

    @classmethod
    def _dropout_args(cls, p, seed, key, n_docs: int = 0):
        """-> thr = round(p * 2^24); ValueError unless p is a real in [0, 1] and seed, key and
        key + n_docs are ints in [0, 2^64)."""
        import numbers
        if isinstance(p, bool) or not isinstance(p, numbers.Real) or not 0 <= p <= 1:   # (a NaN fails the comparison)
            raise ValueError("p is a real number in [0, 1]")
        for name, v in (("seed", seed), ("doc_key / doc_base", key)):
            if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 0 <= int(v) < cls._U64:
                raise ValueError(f"{name} is an int in [0, 2^64)")
        if int(key) + n_docs >= cls._U64:
            raise ValueError("doc_base + len(texts) is below 2^64")
        return int(round(float(p) * (1 << 24)))

    def encode_batch_dropout_np(self, texts: List[str], p: float, seed: int, doc_base: int = 0):
        """-> (ids np.uint32 [total], offsets np.int64 [len(texts) + 1]) as encode_batch_np, each
        candidate merge skipped with probability p; document i draws with (seed, doc_base + i)."""
        import numpy as np
        texts = list(texts)
        thr = self._dropout_args(p, seed, doc_base, len(texts))
        h = self._device()
        data, starts = self._join(texts)
        n, nd = len(data), len(texts)
        ids = np.empty(max(n, 1), dtype=np.uint32)
        offsets = np.zeros(nd + 1, dtype=np.uint64)
        n_out = ctypes.c_size_t(0)
        if nd:
            rc = _lib.lib().bpe_tok_encode_dropout(h, data, n, starts.ctypes.data, nd, thr, int(seed), int(doc_base),
                                                   ids.ctypes.data, ids.size, ctypes.byref(n_out), offsets.ctypes.data)
            _lib.check(rc, "encode_dropout")
        return ids[:n_out.value].copy(), offsets.astype(np.int64)

    def encode_batch_dropout(self, texts: List[str], p: float, seed: int, doc_base: int = 0) -> List[List[int]]:
        """[encode_dropout(t, p, seed, doc_base + i) for i, t in enumerate(texts)] in one library call."""
        ids, offsets = self.encode_batch_dropout_np(texts, p, seed, doc_base)
        flat, off = ids.tolist(), offsets.tolist()
        return [flat[a:b] for a, b in zip(off, off[1:])]

    def encode_dropout(self, text: str, p: float, seed: int, doc_key: int = 0) -> List[int]:
        """encode(text) with BPE-dropout: the ids depend on (seed, doc_key, text) alone."""
        self._dropout_args(p, seed, doc_key, 1)
        return self.encode_batch_dropout_np([text], p, seed, doc_key)[0].tolist()

    def encode_batch_padded_dropout(self, texts: List[str], max_length: int | None = None, *, pad_id: int, p: float,
                                    seed: int, doc_base: int = 0, truncation: str = "right",
                                    padding_side: str = "right", dtype=None):
        """encode_batch_padded with BPE-dropout: -> (tensor [len(texts), T], int32 lengths), both on
        the current device, row i the ids of encode_dropout(texts[i], p, seed, doc_base + i).  The
        text goes to the device once and the ids never leave it (bpe_tok_encode_dropout_device,
        then bpe_ids_pack_rows_device)."""
        texts = list(texts)
        thr = self._dropout_args(p, seed, doc_base, len(texts))
        if truncation not in ("right", "left") or padding_side not in ("right", "left"):
            raise ValueError("truncation and padding_side are 'right' or 'left'")
        if max_length is not None and max_length < 0:
            raise ValueError("max_length is negative")
        import torch
        dtype = torch.int64 if dtype is None else dtype
        if dtype not in (torch.int32, torch.int64):
            raise ValueError("dtype is torch.int32 or torch.int64")
        h = self._device()
        L = _lib.lib()
        data, starts = self._join(texts)
        n, nd = len(data), len(texts)
        dev = torch.device("cuda", torch.cuda.current_device())
        lengths = torch.zeros(nd, dtype=torch.int32, device=dev)
        if nd == 0:
            return torch.empty((0, max_length or 0), dtype=dtype, device=dev), lengths
        stream = torch.cuda.current_stream()
        sp = ctypes.c_void_p(stream.cuda_stream)
        d_ids = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        d_off = torch.zeros(nd + 1, dtype=torch.int64, device=dev)
        if n:
            d_text = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
            stream.synchronize()
            n_out = ctypes.c_size_t(0)
            _lib.check(L.bpe_tok_encode_dropout_device(h, ctypes.c_void_p(d_text.data_ptr()), n, starts.ctypes.data, nd,
                                                       thr, int(seed), int(doc_base), ctypes.c_void_p(d_ids.data_ptr()),
                                                       ctypes.byref(n_out), ctypes.c_void_p(d_off.data_ptr()), sp),
                       "encode_dropout")
        T = int((d_off[1:] - d_off[:-1]).max()) if max_length is None else int(max_length)
        out = torch.empty((nd, T), dtype=dtype, device=dev)
        flags = (1 if truncation == "left" else 0) | (2 if padding_side == "left" else 0)
        stream.synchronize()
        _lib.check(L.bpe_ids_pack_rows_device(ctypes.c_void_p(d_ids.data_ptr()), ctypes.c_void_p(d_off.data_ptr()), nd,
                                              T, int(pad_id), flags, 4 if dtype == torch.int32 else 8,
                                              ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(lengths.data_ptr()),
                                              sp), "pack rows")
        return out, lengths

    def encode_iterable(self, iterable: Iterable[str]) -> Iterator[int]:
        """tokenizer.py:140-150: concatenate items until >= 2 MiB characters, encode each chunk."""
        it = iter(iterable)
        while True:
            text = ""
            for line in it:
                text += line
                if len(text) >= 1024 * 1024 * 2:
                    break
            if not text:
                break
            yield from self.encode(text)

    def _decoder(self):
        if getattr(self, "_dec", None) is None:
            import struct
            ents = [(i, b) for i, b in self.vocab.items() if isinstance(i, int)]
            blob = struct.pack("<I", len(ents)) + b"".join(
                struct.pack("<qI", int(i), len(b)) + bytes(b) for i, b in ents)
            h = ctypes.c_void_p()
            _lib.check(_lib.lib().bpe_dec_create(blob, len(blob), ctypes.byref(h)), "decoder")
            self._dec = h
        return self._dec

    def decode(self, ids: List[int]) -> str:
        """tokenizer.py:155-157: b"".join(self.vocab[i] for i in ids) gathered on the GPU, then
        CPython's UTF-8 decoder with errors="replace" (its replacement rule, exactly)."""
        ids = list(ids)
        for i in ids:   # ids the uint32 device table cannot hold
            if not isinstance(i, int) or i < 0 or i > 0xFFFFFFFF:
                v = self.vocab[i]   # KeyError, as the reference's lookup raises
                if not isinstance(v, (bytes, bytearray)):   # b"".join of a non-bytes value
                    raise TypeError(f"sequence item: expected a bytes-like object, {type(v).__name__} found")
                raise KeyError(i)   # (a non-int key with a bytes value: not decodable here)
        if not ids:
            return ""
        arr = (ctypes.c_uint32 * len(ids))(*ids)
        L = _lib.lib()
        n_out = ctypes.c_size_t(0)
        rc = L.bpe_dec_decode(self._decoder(), arr, len(ids), None, 0, ctypes.byref(n_out))
        if rc != _lib.BPE_E_ARG or n_out.value == 0:   # size query, or KeyError / empty result
            if rc == _lib.BPE_E_KEY:
                raise KeyError(int((L.bpe_last_error() or b"0").decode()))
            _lib.check(rc, "decode")
        buf = (ctypes.c_uint8 * max(n_out.value, 1))()
        _lib.check(L.bpe_dec_decode(self._decoder(), arr, len(ids), buf, n_out.value, ctypes.byref(n_out)),
                   "decode")
        return bytes(buf[:n_out.value]).decode("utf-8", errors="replace")

    # ------------------------------------------------------------------ batch decode
    # decode(r) for every row r in one launch sequence (bpe_dec_decode_batch: the lengths of all
    # ids, one scan, one tiled gather, no size-query pass), the other half of the batch encode.
    # The library returns the rows' bytes concatenated and where each row begins; the string forms
    # slice that buffer and run CPython's decoder with errors="replace" on every slice, so the
    # replacement rule applies per row exactly as in separate decode() calls.  On the current
    # device, like the batch encode.
    def _check_ids(self, ids) -> None:
        """What decode() raises for an id the uint32 device table cannot hold."""
        for i in ids:
            if not isinstance(i, int) or i < 0 or i > 0xFFFFFFFF:
                v = self.vocab[i]   # KeyError, as the reference's lookup raises
                if not isinstance(v, (bytes, bytearray)):
                    raise TypeError(f"sequence item: expected a bytes-like object, {type(v).__name__} found")
                raise KeyError(i)

    def _flatten(self, rows):
        """rows of ids -> (ids np.uint32 [total], offsets np.uint64 [len(rows) + 1]); an id decode()
        would refuse raises what decode() raises, for the first such row."""
        import numpy as np
        rows = [list(r) for r in rows]
        offsets = np.zeros(len(rows) + 1, dtype=np.uint64)
        if rows:
            np.cumsum(np.fromiter(map(len, rows), dtype=np.uint64, count=len(rows)), out=offsets[1:])
        flat = list(itertools.chain.from_iterable(rows))
        ids = None
        if set(map(type, flat)) <= {int}:   # the common case, checked without a Python-level loop
            try:
                a = np.array(flat, dtype=np.int64)
            except OverflowError:
                a = None
            if a is not None and (a.size == 0 or (int(a.min()) >= 0 and int(a.max()) <= 0xFFFFFFFF)):
                ids = a.astype(np.uint32)
        if ids is None:
            for r in rows:
                self._check_ids(r)
            ids = np.array([int(i) for i in flat], dtype=np.int64).astype(np.uint32)   # bool, int subclasses
        return ids, offsets

    @staticmethod
    def _decode_status(rc: int, what: str) -> None:
        if rc == _lib.BPE_E_KEY:   # vocab[i] of an id without an entry
            raise KeyError(int((_lib.lib().bpe_last_error() or b"0").decode()))
        _lib.check(rc, what)

    def _decode_csr(self, ids, offsets, want_token_offsets: bool = False):
        """ids np.uint32, offsets np.uint64 (both contiguous) -> (bytes of all rows, byte offsets
        np.uint64 [rows + 1], token offsets np.uint64 [len(ids) + 1] or None)."""
        import numpy as np
        dec = self._decoder()
        L = _lib.lib()
        n, nr = int(ids.size), int(offsets.size) - 1
        byte_off = np.zeros(nr + 1, dtype=np.uint64)
        tok_off = np.zeros(n + 1, dtype=np.uint64) if want_token_offsets else None
        p, nb = ctypes.c_void_p(), ctypes.c_size_t(0)
        rc = L.bpe_dec_decode_batch(dec, ids.ctypes.data, n, offsets.ctypes.data, nr, ctypes.byref(p), ctypes.byref(nb),
                                    byte_off.ctypes.data, tok_off.ctypes.data if want_token_offsets else None)
        self._decode_status(rc, "decode_batch")
        try:
            data = ctypes.string_at(p, nb.value)
        finally:
            L.bpe_blob_free(p)
        return data, byte_off, tok_off

    def decode_batch_bytes(self, rows) -> List[bytes]:
        """[b"".join(vocab[i] for i in r) for r in rows]: the rows' raw bytes before UTF-8 decoding,
        one library call (see decode_batch)."""
        self._decoder()
        data, byte_off, _ = self._decode_csr(*self._flatten(rows))
        off = byte_off.tolist()
        return [data[a:b] for a, b in zip(off, off[1:])]

    def decode_batch(self, rows) -> List[str]:
        """[decode(r) for r in rows] in one library call, with decode()'s exceptions for the first
        offending row (KeyError(id) for an id without a vocab entry)."""
        return [b.decode("utf-8", errors="replace") for b in self.decode_batch_bytes(rows)]

    def decode_tokens(self, ids) -> List[str]:
        """[decode([i]) for i in ids] in one library call: one row per id."""
        return self.decode_batch([(i,) for i in ids])

    def decode_batch_np(self, ids, offsets, return_token_offsets: bool = False):
        """CSR ids, as encode_batch_np returns them -> (bytes np.uint8 [total], byte_offsets np.int64
        [rows + 1]): row i's bytes are bytes[byte_offsets[i]:byte_offsets[i + 1]].  With
        return_token_offsets also token_offsets np.int64 [len(ids) + 1]: token j's bytes are
        bytes[token_offsets[j]:token_offsets[j + 1]]."""
        import numpy as np
        self._decoder()
        ids, offsets = np.asarray(ids), np.asarray(offsets)
        if ids.ndim != 1 or offsets.ndim != 1 or ids.dtype.kind not in "iu" or offsets.dtype.kind not in "iu":
            raise ValueError("ids and offsets are 1-D integer arrays")
        if ids.dtype != np.uint32:
            bad = np.flatnonzero((ids < 0) | (ids > 0xFFFFFFFF))
            if bad.size:
                raise KeyError(int(ids[bad[0]]))
        if offsets.size == 0 or offsets[0] != 0 or offsets[-1] != ids.size or (np.diff(offsets.astype(np.int64)) < 0).any():
            raise ValueError("offsets start at 0, do not decrease and end at len(ids)")
        data, byte_off, tok_off = self._decode_csr(np.ascontiguousarray(ids, dtype=np.uint32),
                                                   np.ascontiguousarray(offsets, dtype=np.uint64),
                                                   return_token_offsets)
        out = (np.frombuffer(data, dtype=np.uint8).copy(), byte_off.astype(np.int64))
        return out + (tok_off.astype(np.int64),) if return_token_offsets else out

    def decode_batch_padded(self, rows, lengths=None, *, stop_id: int | None = None, include_stop: bool = False,
                            padding_side: str = "right") -> List[str]:
        """A [B, T] torch.int32 / torch.int64 tensor of ids -> B strings; the ids never visit the
        host (bpe_dec_decode_rows_device), only the bytes and the row offsets come back.  Row i is
        decoded over its kept span: its first lengths[i] entries (padding_side="left": its last),
        or all T when lengths is None; with stop_id, up to the first entry equal to it
        (include_stop: that entry too).  What lies outside the span is never looked at, so any pad
        value may stand there.  encode_batch_padded's (tensor, lengths) decode back with the same
        padding_side.  A tensor on the current GPU is used in place (made contiguous if it is
        not); anything else is moved there."""
        import torch
        if padding_side not in ("right", "left"):
            raise ValueError("padding_side is 'right' or 'left'")
        if not isinstance(rows, torch.Tensor):
            rows = torch.as_tensor(rows)
        if rows.dtype not in (torch.int32, torch.int64):
            raise ValueError("rows is a torch.int32 or torch.int64 tensor")
        if rows.dim() != 2:
            raise ValueError("rows is a 2-D tensor [B, T]")
        if stop_id is not None and not 0 <= int(stop_id) <= 0xFFFFFFFF:
            raise ValueError("stop_id is an id in [0, 2^32) or None")
        B, T = int(rows.shape[0]), int(rows.shape[1])
        dec = self._decoder()
        L = _lib.lib()
        import numpy as np
        dev = torch.device("cuda", torch.cuda.current_device())
        rows = rows.to(dev).contiguous()
        if lengths is not None:
            lengths = torch.as_tensor(lengths).to(device=dev, dtype=torch.int32).contiguous()
            if lengths.dim() != 1 or lengths.shape[0] != B:
                raise ValueError("lengths has one entry per row")
        stream = torch.cuda.current_stream()
        stream.synchronize()   # the rows are complete before the library's stream reads them
        byte_off = np.zeros(B + 1, dtype=np.uint64)
        p, nb = ctypes.c_void_p(), ctypes.c_size_t(0)
        flags = (1 if include_stop else 0) | (2 if padding_side == "left" else 0)
        rc = L.bpe_dec_decode_rows_device(dec, ctypes.c_void_p(rows.data_ptr()), rows.element_size(), B, T,
                                          ctypes.c_void_p(lengths.data_ptr()) if lengths is not None else None,
                                          -1 if stop_id is None else int(stop_id), flags, ctypes.byref(p),
                                          ctypes.byref(nb), byte_off.ctypes.data, ctypes.c_void_p(stream.cuda_stream))
        if rc == _lib.BPE_E_ARG:
            raise ValueError((L.bpe_last_error() or b"").decode("utf-8", "replace"))
        self._decode_status(rc, "decode_batch_padded")
        try:
            data = ctypes.string_at(p, nb.value)
        finally:
            L.bpe_blob_free(p)
        off = byte_off.tolist()
        return [data[a:b].decode("utf-8", errors="replace") for a, b in zip(off, off[1:])]

    def save(self, path: str, prefix: str = ""):
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, prefix + "-vocab.pkl"), "wb+") as f:
            pickle.dump(self.vocab, f)
        with open(os.path.join(path, prefix + "-merges.pkl"), "wb+") as f:
            pickle.dump(self.merges, f)
