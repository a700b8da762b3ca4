"""Dataset encoder -- drop-in for reference models/tokenizer/encode.py (and the memmap input of
train.py:230-232).

The reference reads the split in text mode 1 M characters at a time, encodes every piece with
Tokenizer.encode_iterable([piece]) and saves np.array(ids, dtype=np.uint16) with
torch.save(..., pickle_protocol=4).  Here the whole file goes to the device once:

    bytes -> bpe_text_prepare_device    (strict UTF-8 + universal newlines: the text-mode read)
          -> bpe_utf8_chunk_starts_device (where each 1 M-character piece starts)
          -> bpe_tok_encode_chunks_device (one launch sequence for all pieces; a piece boundary
                                          ends every pre-token and no special straddles it, so
                                          the ids equal the per-piece encodes, concatenated)
          -> bpe_ids_to_u16_device        (np.uint16, refusing ids > 65535 instead of wrapping)

and the uint16 ids come back to the host once.  Output formats: "pt" (the reference's file,
torch.save of the np.uint16 array) and "bin" (raw uint16, what train.py's np.memmap reads).

(The reference's loop passes a one-element LIST to encode_iterable, which re-iterates it
forever -- tokenizer.py:140-150; DESIGN.md section 7.  The ids written here are the ones the
loop would produce if it terminated.)
"""
from __future__ import annotations

import argparse
import ctypes
import os
import stat

import numpy as np

from . import _lib
from . import utf8 as _utf8
from .tokenizer import Tokenizer

fname = {   # encode.py:8-15
    "tiny/train": "TinyStoriesV2-GPT4-train.txt",
    "tiny/valid": "TinyStoriesV2-GPT4-valid.txt",
    "owt/train": "owt_train.txt",
    "owt/valid": "owt_valid.txt",
    "corpus/train": "corpus.en",
    "corpus/valid": "corpus.en",
}

CHARS_PER_PIECE = 1024 * 1024   # encode.py:33 f.read(1024 * 1024)


def _prepare_repaired(raw, mode: int, errors: str, path):
    """The non-strict text-mode read of a tensor whose strict read failed: a new tensor holding
    the repaired, newline-translated text, and its length.  raw is not modified."""
    import torch
    L = _lib.lib()
    n = raw.numel()
    need, st = ctypes.c_size_t(0), _lib.Utf8Stats()
    _lib.check(L.bpe_text_prepare_device_ex(ctypes.c_void_p(raw.data_ptr()), n, mode, None, 0, ctypes.byref(need),
                                            ctypes.byref(st), None), "read")
    out = torch.empty(max(need.value, 1), dtype=torch.uint8, device=raw.device)
    m = ctypes.c_size_t(0)
    _lib.check(L.bpe_text_prepare_device_ex(ctypes.c_void_p(raw.data_ptr()), n, mode, ctypes.c_void_p(out.data_ptr()),
                                            need.value, ctypes.byref(m), ctypes.byref(st), None), "read")
    d = _utf8.stats_dict(st)
    _utf8.note(errors, d["n_units"], d["n_bytes"], (path, d["first"]) if d["first"] is not None else None)
    return out, m.value


def encode_device_u16(tokenizer: Tokenizer, raw, chars_per_piece: int = CHARS_PER_PIECE, errors: str = "strict",
                      _path=None) -> np.ndarray:
    """The reference's encode.py ids for the raw file bytes held in the device tensor `raw`
    (uint8; overwritten by the text-mode read), as np.uint16 in host memory.  errors "replace" or
    "ignore": bytes the strict read refuses are repaired first, as open(..., errors=...) reads them."""
    mode = _utf8.mode_of(errors)
    import torch
    L = _lib.lib()
    n = raw.numel()
    if mode:
        _utf8.note(errors, 0, 0, None)
    if n == 0:
        return np.zeros(0, dtype=np.uint16)
    m = ctypes.c_size_t(0)
    rc = L.bpe_text_prepare_device(ctypes.c_void_p(raw.data_ptr()), n, ctypes.c_void_p(raw.data_ptr()),
                                   ctypes.byref(m), None)
    if mode and rc == _lib.BPE_E_UTF8:   # validation failed before anything was written: repair, then read
        raw, m = _prepare_repaired(raw, mode, errors, _path)
        if m == 0:
            return np.zeros(0, dtype=np.uint16)
    else:
        _lib.check(rc, "read")
        m = m.value
    ns = ctypes.c_size_t(0)
    _lib.check(L.bpe_utf8_chunk_starts_device(ctypes.c_void_p(raw.data_ptr()), m, chars_per_piece, None, 0,
                                              ctypes.byref(ns), None), "chunk starts")
    starts = (ctypes.c_uint64 * max(ns.value, 1))()
    _lib.check(L.bpe_utf8_chunk_starts_device(ctypes.c_void_p(raw.data_ptr()), m, chars_per_piece, starts,
                                              ns.value, ctypes.byref(ns), None), "chunk starts")
    ids = torch.empty(max(m, 1), dtype=torch.int32, device="cuda")
    n_ids = ctypes.c_size_t(0)
    _lib.check(L.bpe_tok_encode_chunks_device(tokenizer._device(), ctypes.c_void_p(raw.data_ptr()), m, starts,
                                              ns.value, ctypes.c_void_p(ids.data_ptr()), ctypes.byref(n_ids),
                                              None), "encode")
    k = n_ids.value
    out16 = torch.empty(max(k, 1), dtype=torch.int16, device="cuda")
    _lib.check(L.bpe_ids_to_u16_device(ctypes.c_void_p(ids.data_ptr()), k, ctypes.c_void_p(out16.data_ptr()),
                                       None), "uint16 ids")
    del ids
    host = np.empty(k, dtype=np.uint16)
    if k:
        _lib.check(L.bpe_copy_to_host(ctypes.c_void_p(out16.data_ptr()), 2 * k, host.ctypes.data), "copy")
    return host


def encode_bytes_u16(tokenizer: Tokenizer, data: bytes, chars_per_piece: int = CHARS_PER_PIECE,
                     errors: str = "strict", _path=None) -> np.ndarray:
    """The reference's encode.py ids for a file whose raw bytes are `data`, as np.uint16."""
    mode = _utf8.mode_of(errors)
    import torch
    if len(data) == 0:
        if mode:
            _utf8.note(errors, 0, 0, None)
        return np.zeros(0, dtype=np.uint16)
    raw = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda")
    torch.cuda.synchronize()
    return encode_device_u16(tokenizer, raw, chars_per_piece, errors, _path)


def read_file_device(path):
    """A regular file's raw bytes in HBM (uint8 tensor) through the library's reader: pinned
    staging buffers filled by a pool of pread threads, each DMA'd while the next is read.  None
    for a file that is not regular (a pipe, FIFO or device): the caller reads it itself."""
    import torch
    if not stat.S_ISREG(os.stat(path).st_mode):   # missing: FileNotFoundError, as open() raises
        return None
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    p = os.fsencode(os.fspath(path))
    _lib.check(L.bpe_read_file_device(p, None, 0, ctypes.byref(n)), "read")
    raw = torch.empty(max(n.value, 1), dtype=torch.uint8, device="cuda")[:n.value]
    if n.value:
        _lib.check(L.bpe_read_file_device(p, ctypes.c_void_p(raw.data_ptr()), n.value, ctypes.byref(n)), "read")
    return raw


last_phases_ms = {}   # the last encode_file's read / decode / encode / copy times (library clock)


def encode_file_native(tokenizer: Tokenizer, path, chars_per_piece: int = CHARS_PER_PIECE) -> np.ndarray:
    """A regular file through bpe_tok_encode_file_u16: read into HBM by the library's reader,
    decoded, pieces, encoded straight to uint16 in a device buffer the tokenizer keeps, and copied
    into host memory by copier threads -- no intermediate uint32 ids, no per-call device arrays."""
    L = _lib.lib()
    n = os.stat(path).st_size
    host = np.empty(max(n, 1), dtype=np.uint16)   # ids <= bytes; pages are touched only as written
    k = ctypes.c_size_t(0)
    ph = (ctypes.c_double * 4)()
    _lib.check(L.bpe_tok_encode_file_u16(tokenizer._device(), os.fsencode(os.fspath(path)), chars_per_piece,
                                         host.ctypes.data, host.size, ctypes.byref(k), ph), "encode file")
    last_phases_ms.clear()
    last_phases_ms.update(read=ph[0], decode=ph[1], encode=ph[2], copy=ph[3])
    return host[:k.value]


def encode_file(tokenizer: Tokenizer, input_path, output_path=None, fmt: str = "pt",
                chars_per_piece: int = CHARS_PER_PIECE, keep_device_buffers: bool = False,
                errors: str = "strict") -> np.ndarray:
    """Encode a text file like encode.py:main; write it if output_path is given.  The device
    buffers of the bulk encoder (about 3 bytes of HBM per file byte) are released afterwards
    unless keep_device_buffers (several files in a row: re-allocating tens of GB costs the driver
    up to seconds per call).  errors "replace" or "ignore": the file is read as open(path,
    encoding="utf-8", errors=...) reads it; it then goes to the device whole and through the
    text-prepare step with that mode (encode_device_u16), not through the overlapped reader."""
    if _utf8.mode_of(errors):
        raw = read_file_device(input_path)
        if raw is None:
            with open(input_path, "rb") as f:
                pt = encode_bytes_u16(tokenizer, f.read(), chars_per_piece, errors, os.fspath(input_path))
        else:
            pt = encode_device_u16(tokenizer, raw, chars_per_piece, errors, os.fspath(input_path))
    elif stat.S_ISREG(os.stat(input_path).st_mode):   # missing: FileNotFoundError, as open() raises
        try:
            pt = encode_file_native(tokenizer, input_path, chars_per_piece)
        finally:
            if not keep_device_buffers:
                tokenizer.release_device_buffers()
    else:
        with open(input_path, "rb") as f:
            data = f.read()
        pt = encode_bytes_u16(tokenizer, data, chars_per_piece)
    if output_path is not None:
        if fmt == "pt":
            import torch
            torch.save(pt, output_path, pickle_protocol=4)   # encode.py:38
        elif fmt == "bin":
            pt.tofile(output_path)                           # np.memmap(path, np.uint16, "r")
        else:
            raise ValueError(f"unknown format {fmt!r}")
    return pt


MIN_WINDOW_BYTES = 64 * 1024    # as WordCounter.add_file
DEFAULT_WINDOW_BYTES = 1 << 30  # a choice, not a measured optimum


def _largest_id(tokenizer: Tokenizer) -> int:
    """The largest id the tokenizer can emit: a vocab entry's or a special's."""
    ids = [i for b, i in tokenizer.vocab_inv.items() if isinstance(b, (bytes, bytearray)) and isinstance(i, int)]
    return max(ids) if ids else 0


def _same_file(a, b) -> bool:
    a, b = os.fspath(a), os.fspath(b)
    if os.path.realpath(a) == os.path.realpath(b):
        return True
    try:
        return os.path.samefile(a, b)
    except OSError:
        return False


def encode_files(tokenizer: Tokenizer, paths, output_path, *, dtype=None, window_bytes=None,
                 chars_per_piece: int = CHARS_PER_PIECE, separator=None, index_path=None,
                 count_ids: bool = False, keep_device_buffers: bool = False, errors: str = "strict") -> dict:
    """Encode many text files of any size into one token file.

    Each file is encoded exactly as encode_file encodes it alone (text-mode read, pieces of
    chars_per_piece characters counted from the start of that file, each piece on its own); the
    ids are concatenated in the order of `paths` and written to output_path as raw little-endian
    ids, what np.memmap(output_path, dtype) reads.  The raw bytes of each file are read in
    consecutive ranges of exactly window_bytes (None: 1 GiB; at least 64 KiB); neither HBM nor
    host memory holds anything proportional to a file's size (the exact bound: include/bpe355.h,
    bpe_tok_encode_files).  Input that is not a regular file (a FIFO) is read to its end into
    host memory first, as encode_file does.

    dtype: np.uint16 or np.uint32; None picks uint16 when every id the tokenizer can emit is below
    65536, else uint32.  A forced uint16 with a wider id raises RuntimeError (BPE_E_LIMIT).
    separator (a special-token string of the tokenizer, or an int id) with index_path: the
    positions in the whole stream where that id stands, ascending, raw little-endian uint64.
    count_ids: the result carries id_counts, np.uint64 of length largest emittable id + 1,
    accumulated on the device.

    Raises FileNotFoundError for a missing file and UnicodeDecodeError (position in that raw file,
    the message names the file) for ill-formed UTF-8; after any error output_path and index_path
    are as they were before the call.  Runs on the current device (set_num_gpus does not apply).
    The device buffers are released afterwards unless keep_device_buffers.

    errors "replace" or "ignore": a raw range with ill-formed UTF-8 is repaired on the device as
    open(path, encoding="utf-8", errors=...) decodes it (pieces count characters of the repaired
    text, U+FFFD is one); the result then also carries n_replaced (spans replaced or dropped) and
    file_replaced (np.int64, one entry per path), and last_utf8_errors() reports the call.

    Returns a dict: n_ids, dtype, file_offsets (np.int64, len(paths) + 1), n_bytes, n_pieces,
    n_windows, max_window_bytes, n_separators, n_grows, device_bytes, the busy milliseconds
    read_ms, decode_ms, encode_ms, write_ms and stats_ms, and id_counts when asked for."""
    mode = _utf8.mode_of(errors)
    paths = [os.fspath(p) for p in paths]
    if dtype is not None:
        try:
            dtype = np.dtype(dtype)
        except TypeError as e:
            raise ValueError(f"dtype must be np.uint16 or np.uint32, not {dtype!r}") from e
        if dtype not in (np.dtype(np.uint16), np.dtype(np.uint32)):
            raise ValueError(f"dtype must be np.uint16 or np.uint32, not {dtype}")
    if window_bytes is not None and int(window_bytes) < MIN_WINDOW_BYTES:
        raise ValueError(f"window_bytes must be at least {MIN_WINDOW_BYTES}")
    if int(chars_per_piece) < 1:
        raise ValueError("chars_per_piece must be at least 1")
    if (separator is None) != (index_path is None):
        raise ValueError("separator and index_path go together")
    sep_id = 0
    if separator is not None:
        if isinstance(separator, str):
            if separator not in tokenizer.special_tokens:
                raise ValueError(f"{separator!r} is not a special token of the tokenizer")
            sep_id = tokenizer.vocab_inv[separator.encode("utf-8")]
        else:
            sep_id = int(separator)
            if sep_id < 0:
                raise ValueError("a separator id is not negative")
    outs = [output_path] + ([index_path] if index_path is not None else [])
    if index_path is not None and _same_file(output_path, index_path):
        raise ValueError("output_path and index_path are the same file")
    for o in outs:
        for p in paths:
            if _same_file(o, p):
                raise ValueError(f"{os.fspath(o)!r} is both an input and an output")
    for p in paths:
        os.stat(p)   # missing: FileNotFoundError, as open() raises, before the device is touched
    top = _largest_id(tokenizer)
    if dtype is None:
        dtype = np.dtype(np.uint16 if top < 65536 else np.uint32)

    L = _lib.lib()
    opts = _lib.DatasetOpts(int(chars_per_piece), int(window_bytes or 0), dtype.itemsize,
                            1 if separator is not None else 0, sep_id,
                            os.fsencode(os.fspath(index_path)) if index_path is not None else None)
    arr = (ctypes.c_char_p * max(1, len(paths)))(*[os.fsencode(p) for p in paths])
    offsets = np.zeros(len(paths) + 1, dtype=np.uint64)
    counts = np.zeros(top + 1, dtype=np.uint64) if count_ids else None
    st = _lib.DatasetStats()
    fix, fix_file, fix_units = _lib.Utf8Stats(), ctypes.c_uint64(0), np.zeros(max(1, len(paths)), dtype=np.uint64)
    try:
        if mode:
            _lib.check(L.bpe_tok_set_errors(tokenizer._device(), mode), "encode files")
        rc = L.bpe_tok_encode_files(tokenizer._device(), arr, len(paths), os.fsencode(os.fspath(output_path)),
                                    ctypes.byref(opts), offsets.ctypes.data,
                                    counts.ctypes.data if count_ids else None, counts.size if count_ids else 0,
                                    ctypes.byref(st))
        _lib.check(rc, "encode files")
        if mode:
            _lib.check(L.bpe_tok_utf8_report(tokenizer._device(), ctypes.byref(fix), ctypes.byref(fix_file),
                                             fix_units.ctypes.data, len(paths)), "encode files")
    finally:
        if mode:
            L.bpe_tok_set_errors(tokenizer._device(), 0)
        if not keep_device_buffers:
            tokenizer.release_device_buffers()
    out = st.as_dict()
    if mode:
        d = _utf8.stats_dict(fix)
        _utf8.note(errors, d["n_units"], d["n_bytes"],
                   (paths[fix_file.value], d["first"]) if d["first"] is not None else None)
        out["n_replaced"] = d["n_units"]
        out["file_replaced"] = fix_units[:len(paths)].astype(np.int64)
    out["dtype"] = dtype
    out["file_offsets"] = offsets.astype(np.int64)
    if count_ids:
        out["id_counts"] = counts
    return out


def _ids_arg(ids):
    import torch
    sizes = {torch.int16: 2, torch.uint16: 2, torch.int32: 4, torch.int64: 8}
    if not (isinstance(ids, torch.Tensor) and ids.is_cuda and ids.dim() == 1 and ids.is_contiguous()
            and ids.dtype in sizes):
        raise ValueError("ids must be a contiguous 1-D cuda tensor of int16, uint16, int32 or int64")
    return sizes[ids.dtype]


def _check_ids(rc: int, what: str):
    if rc == _lib.BPE_E_ARG:   # an id outside the table or outside [0, 2^32)
        raise ValueError((_lib.lib().bpe_last_error() or b"").decode("utf-8", "replace"))
    _lib.check(rc, what)


def id_counts(ids, size: int, out=None):
    """out[id] += occurrences of id in `ids` (a contiguous 1-D cuda tensor of int16/uint16, int32 or
    int64; the bits of int16 and int32 are read as unsigned, an int64 entry outside [0, 2^32) is an
    error), as a uint64 tensor of `size` entries on the device (out: such a tensor to add into,
    uint64 or int64 bits; None: zeros).  An id >= size raises ValueError naming the smallest one,
    and `out` is not to be used after that."""
    import torch
    eb = _ids_arg(ids)
    size = int(size)
    if size < 1 or size > 1 << 32:
        raise ValueError("size must be in [1, 2^32]")
    if out is None:
        out = torch.zeros(size, dtype=torch.int64, device=ids.device).view(torch.uint64)
    elif not (isinstance(out, torch.Tensor) and out.device == ids.device and out.dim() == 1 and out.is_contiguous()
              and out.numel() == size and out.dtype in (torch.uint64, torch.int64)):
        raise ValueError("out must be a contiguous uint64 cuda tensor of `size` entries beside ids")
    with torch.cuda.device(ids.device):
        torch.cuda.current_stream().synchronize()
        _check_ids(_lib.lib().bpe_ids_histogram_device(ctypes.c_void_p(ids.data_ptr()), ids.numel(), eb,
                                                       ctypes.c_void_p(out.data_ptr()), size, None), "id counts")
    return out


def id_positions(ids, value: int, base: int = 0):
    """base + i for every i with ids[i] == value, ascending, as an int64 tensor on the device
    (ids as for id_counts)."""
    import torch
    eb = _ids_arg(ids)
    value, base = int(value), int(base)
    if value < 0 or base < 0:
        raise ValueError("value and base are not negative")
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    with torch.cuda.device(ids.device):
        torch.cuda.current_stream().synchronize()
        _check_ids(L.bpe_ids_find_device(ctypes.c_void_p(ids.data_ptr()), ids.numel(), eb, value, base, None, 0,
                                         ctypes.byref(n), None), "id positions")
        pos = torch.empty(n.value, dtype=torch.int64, device=ids.device)
        if n.value:
            _check_ids(L.bpe_ids_find_device(ctypes.c_void_p(ids.data_ptr()), ids.numel(), eb, value, base,
                                             ctypes.c_void_p(pos.data_ptr()), n.value, ctypes.byref(n), None),
                       "id positions")
    return pos


def main(dataset: str, split: str, fmt: str = "pt"):
    """encode.py:18-38 with the same paths."""
    if dataset == "corpus":
        input_file = "tests/fixtures/corpus.en"
    else:
        input_file = f"/data/{fname[dataset + '/' + split]}"
    tokenizer = Tokenizer.from_files(
        vocab_filepath=f"data/tokenizer/{dataset}-vocab.pkl",
        merges_filepath=f"data/tokenizer/{dataset}-merges.pkl",
        special_tokens=["<|endoftext|>"],
    )
    ext = "pt" if fmt == "pt" else "bin"
    encode_file(tokenizer, input_file, f"data/tokenizer/{dataset}-tokens-{split}.{ext}", fmt=fmt)


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--dataset", type=str)
    parser.add_argument("--split", type=str)
    parser.add_argument("--format", type=str, default="pt", choices=["pt", "bin"])
    args = parser.parse_args()
    main(args.dataset, args.split, args.format)
