"""The batch loader: windows of a token file -> the input and target tensors of a training step.

    from bpe_amd.batches import load_batch          # drop-in for models/util.py:37-57
    x, y = load_batch(dataset, batch_size, context_length, device)

    store = TokenStore.from_file("train.bin", np.uint16, index_path="train.idx")
    b = store.sample(128, 1024, positions=True, doc_ids=True, ignore_index=-100)
    b.inputs, b.targets, b.positions, b.doc_ids, b.starts

The reference draws the starts with torch.randint, slices the memmap row by row in Python into two
float64 arrays and copies both to the device.  Here one kernel (csrc/batch.hip) reads each row's
context_length + 1 ids once and writes both matrices; with the separator positions that encode_files
writes (train.idx) it also gives every token's position inside its document and the row's segment
ids.  A store is either resident (the ids live in HBM) or in host mode (a NumPy array or memmap;
the rows are gathered into pinned memory by a few threads, copied once and cut by the same kernel).
There is no CPU fallback.
"""
from __future__ import annotations

import collections
import ctypes
import operator
import os
import re
import threading

import numpy as np

from . import _lib

BatchResult = collections.namedtuple("BatchResult", "inputs targets positions doc_ids starts")

_NP_DTYPES = {np.dtype(np.uint16): (np.dtype(np.uint16), 2), np.dtype(np.int16): (np.dtype(np.uint16), 2),
              np.dtype(np.uint32): (np.dtype(np.uint32), 4), np.dtype(np.int32): (np.dtype(np.uint32), 4)}

_stages = {}                 # device index -> (staging handle, lock): shared by every host-mode store
_stages_lock = threading.Lock()


def _np_dtype(dtype):
    try:
        dt = np.dtype(dtype)
    except TypeError as e:
        raise ValueError(f"dtype must be uint16, int16, uint32 or int32, not {dtype!r}") from e
    if dt not in _NP_DTYPES:
        raise ValueError(f"dtype must be uint16, int16, uint32 or int32, not {dt}")
    return dt


def _stage(index: int):
    """The staging handle of a device (created on first use, with that device current)."""
    with _stages_lock:
        if index not in _stages:
            h = ctypes.c_void_p()
            _lib.check(_lib.lib().bpe_batch_stage_create(ctypes.byref(h)), "batch stage")
            _stages[index] = (h, threading.Lock())
        return _stages[index]


def release_staging():
    """Free the pinned and device buffers of the host-mode path (they are kept between calls)."""
    with _stages_lock:
        for h, lock in _stages.values():
            with lock:
                _lib.lib().bpe_batch_stage_free(h)
        _stages.clear()


def _read_index(index_path, n_ids: int) -> np.ndarray:
    size = os.stat(index_path).st_size
    if size % 8:
        raise ValueError(f"{os.fspath(index_path)!r} is not a whole number of uint64 positions ({size} bytes)")
    sep = np.fromfile(index_path, dtype=np.uint64)
    if sep.size and (int(sep[-1]) >= n_ids or (sep.size > 1 and not bool(np.all(sep[1:] > sep[:-1])))):
        raise ValueError(f"{os.fspath(index_path)!r} does not hold ascending positions below {n_ids}")
    return sep


class TokenStore:
    """A token stream to cut batches from.  Build one with from_file, from_tensor or from_array."""

    def __init__(self, ids, n_ids, dtype, elem_bytes, device, sep_host=None, sep_dev=None, separator_id=None):
        self._ids = ids                    # cuda tensor (resident) or ndarray (host mode)
        self._resident = not isinstance(ids, np.ndarray)
        self._n = int(n_ids)
        self._dtype = dtype
        self._eb = elem_bytes
        self._device = device              # torch.device; host mode: None until the first batch
        self._sep_host = sep_host          # np.uint64 positions, or None
        self._sep_dev = sep_dev            # the same on the device (int64 bits), uploaded on first use
        self._sep_id = separator_id
        self._status = None
        self._host_starts = collections.deque(maxlen=4)
        self._closed = False

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_file(cls, path, dtype, *, index_path=None, separator_id=None, resident=True, device=None):
        """The raw ids np.memmap(path, dtype) reads (what encode_files writes).

        resident=True brings the file into HBM with the library's file reader; resident=False keeps
        an np.memmap and serves batches through the staging path.  The separator positions come from
        index_path (uint64, as encode_files writes them); with separator_id alone and a resident
        store they are found on the device.  With both and a resident store the two are compared
        once, here, and a mismatch is a ValueError; a host-mode store trusts its index file."""
        dt = _np_dtype(dtype)
        size = os.stat(path).st_size
        unsigned, eb = _NP_DTYPES[dt]
        if size % eb:
            raise ValueError(f"{os.fspath(path)!r} holds {size} bytes, not a whole number of {dt} ids")
        n = size // eb
        sep_id = _separator_arg(separator_id)
        sep_host = _read_index(index_path, n) if index_path is not None else None
        if not resident:
            ids = np.memmap(path, dtype=unsigned, mode="r") if n else np.zeros(0, dtype=unsigned)
            return cls(ids, n, unsigned, eb, _device_arg(device), sep_host=sep_host, separator_id=sep_id)
        import torch
        dev = _device_arg(device) or torch.device("cuda", torch.cuda.current_device())
        with torch.cuda.device(dev):
            raw = torch.empty(max(size, 2 * eb), dtype=torch.uint8, device=dev)
            if size:
                got = ctypes.c_size_t(0)
                _lib.check(_lib.lib().bpe_read_file_device(os.fsencode(os.fspath(path)), ctypes.c_void_p(raw.data_ptr()),
                                                           size, ctypes.byref(got)), "read")
                if got.value != size:
                    raise OSError(f"{os.fspath(path)!r} changed size while it was read")
            ids = raw.view(torch.int16 if eb == 2 else torch.int32)[:n]
        store = cls(ids, n, unsigned, eb, dev, sep_host=sep_host, separator_id=sep_id)
        store._finish_separators(f"{os.fspath(index_path)!r}" if index_path is not None else None)
        return store

    @classmethod
    def from_tensor(cls, ids, *, index_path=None, separator_id=None):
        """A contiguous 1-D cuda tensor of uint16, int16 (bits read as unsigned) or int32; it may be
        a slice that starts at any element."""
        import torch
        sizes = {torch.int16: 2, torch.uint16: 2, torch.int32: 4}
        if not (isinstance(ids, torch.Tensor) and ids.is_cuda and ids.dim() == 1 and ids.is_contiguous()
                and ids.dtype in sizes):
            raise ValueError("ids must be a contiguous 1-D cuda tensor of uint16, int16 or int32")
        eb = sizes[ids.dtype]
        sep_id = _separator_arg(separator_id)
        sep_host = _read_index(index_path, ids.numel()) if index_path is not None else None
        store = cls(ids, ids.numel(), np.dtype(np.uint16 if eb == 2 else np.uint32), eb, ids.device,
                    sep_host=sep_host, separator_id=sep_id)
        store._finish_separators(f"{os.fspath(index_path)!r}" if index_path is not None else None)
        return store

    @classmethod
    def from_array(cls, array, *, index_path=None, separator_id=None, device=None):
        """Host mode: a 1-D C-contiguous NumPy array or memmap of uint16, int16, uint32 or int32.  The
        separator positions, if any, come from index_path and are trusted."""
        if not isinstance(array, np.ndarray) or array.ndim != 1 or array.dtype not in _NP_DTYPES \
                or not array.flags.c_contiguous:
            raise ValueError("array must be a 1-D C-contiguous NumPy array of uint16, int16, uint32 or int32")
        unsigned, eb = _NP_DTYPES[array.dtype]
        sep_host = _read_index(index_path, array.size) if index_path is not None else None
        return cls(array, array.size, unsigned, eb, _device_arg(device), sep_host=sep_host,
                   separator_id=_separator_arg(separator_id))

    def _finish_separators(self, index_name):
        """Resident store: find the separator on the device and hold it against the index file."""
        import torch
        if self._sep_id is None or (self._eb == 2 and self._sep_id > 0xFFFF):
            if self._sep_id is not None and self._sep_host is None:
                self._sep_host = np.zeros(0, dtype=np.uint64)   # an id no element can hold
            return
        from .encode import id_positions
        found = id_positions(self._ids, self._sep_id) if self._n else torch.zeros(0, dtype=torch.int64,
                                                                                 device=self._device)
        if self._sep_host is not None:
            given = torch.from_numpy(self._sep_host.view(np.int64)).to(self._device)
            if given.shape != found.shape or not bool(torch.equal(given, found)):
                raise ValueError(f"{index_name} does not hold the positions of id {self._sep_id} in the token "
                                 f"file: {given.numel()} entries against {found.numel()} found")
        else:
            self._sep_host = found.cpu().numpy().view(np.uint64)
        self._sep_dev = found

    # ------------------------------------------------------------------ properties
    @property
    def n_ids(self) -> int:
        return self._n

    def __len__(self) -> int:
        return self._n

    @property
    def dtype(self):
        """np.uint16 or np.uint32: how the ids are read."""
        return self._dtype

    @property
    def resident(self) -> bool:
        return self._resident

    @property
    def device(self):
        return self._device

    @property
    def separator_id(self):
        return self._sep_id

    @property
    def n_docs(self):
        """How many separators the stream holds (documents ended); None without separator positions."""
        return None if self._sep_host is None else int(self._sep_host.size)

    @property
    def separator_positions(self):
        """np.uint64, ascending; None without an index."""
        return self._sep_host

    @property
    def device_bytes(self) -> int:
        """Bytes of HBM the store itself holds: the resident ids and the uploaded index."""
        b = self._ids.numel() * self._eb if self._resident and self._ids is not None else 0
        if self._sep_dev is not None:
            b += self._sep_dev.numel() * 8
        return b

    def close(self):
        self._ids = None
        self._sep_dev = None
        self._status = None
        self._host_starts.clear()
        self._closed = True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    # ------------------------------------------------------------------ batches
    def batch(self, starts, context_length, *, dtype=None, targets=True, positions=False, doc_ids=False,
              ignore_index=None):
        """inputs[r, t] = ids[starts[r] + t] and targets[r, t] = ids[starts[r] + t + 1] as [B, T]
        tensors of `dtype` (torch.int64, the default, or torch.int32) on the store's device.

        positions (int64): the token's index inside its document; doc_ids (int32): segment ids that
        start at 0 in every row.  Both need separator positions.  ignore_index: targets[r, t] is set
        to it where inputs[r, t] is the separator (needs separator_id).  What was not asked for is
        None in the result (inputs, targets, positions, doc_ids, starts).

        starts: a list, a NumPy array or a CPU tensor is range-checked here and the call then only
        enqueues on torch's current stream; a cuda tensor is checked by the kernel, which costs one
        8-byte read-back and a stream synchronisation.  Either way an out-of-range start is an
        IndexError naming the row and the start.  int32 output from a uint32 stream is checked for
        ids from 2^31 on in the same way (RuntimeError naming the smallest one)."""
        return self._batch(starts, context_length, dtype, targets, positions, doc_ids, ignore_index, checked=False)

    def sample(self, batch_size, context_length, *, generator=None, dtype=None, targets=True, positions=False,
               doc_ids=False, ignore_index=None):
        """batch() at batch_size uniformly drawn starts; the result also carries `starts`.  A resident
        store draws them on its device (torch.randint with device=; generator: a generator of that
        device), so nothing crosses the bus and nothing synchronises; a host-mode store draws them on
        the CPU, where the rows are gathered."""
        import torch
        T = _context_arg(context_length)
        B = operator.index(batch_size)
        if B < 0:
            raise ValueError("batch_size is not negative")
        self._check_options(dtype, targets, positions, doc_ids, ignore_index)
        high = self._n - T - (1 if targets else 0) + 1
        if self._resident:
            self._open()
            starts = torch.randint(high, (B,), generator=generator, device=self._device, dtype=torch.int64)
        else:
            starts = torch.randint(high, (B,), generator=generator, dtype=torch.int64)
        return self._batch(starts, T, dtype, targets, positions, doc_ids, ignore_index, checked=True)

    def _open(self):
        if self._closed:
            raise ValueError("the store is closed")

    def _check_options(self, dtype, targets, positions, doc_ids, ignore_index):
        import torch
        if dtype is not None and dtype not in (torch.int32, torch.int64):
            raise ValueError(f"dtype must be torch.int32 or torch.int64, not {dtype!r}")
        if (positions or doc_ids) and self._sep_host is None:
            raise ValueError("positions and doc_ids need separator positions (index_path or separator_id)")
        if ignore_index is not None:
            if not targets:
                raise ValueError("ignore_index applies to targets")
            if self._sep_id is None:
                raise ValueError("ignore_index needs the store's separator_id")
            lo, hi = (-2 ** 31, 2 ** 31 - 1) if dtype == torch.int32 else (-2 ** 63, 2 ** 63 - 1)
            if not lo <= operator.index(ignore_index) <= hi:
                raise ValueError(f"ignore_index {ignore_index} does not fit the output dtype")

    def _batch(self, starts, context_length, dtype, targets, positions, doc_ids, ignore_index, checked):
        import torch
        self._open()
        T = _context_arg(context_length)
        self._check_options(dtype, targets, positions, doc_ids, ignore_index)
        dtype = dtype or torch.int64
        limit = self._n - T - (1 if targets else 0)   # the last valid start
        on_device = isinstance(starts, torch.Tensor) and starts.is_cuda
        if on_device:
            if starts.dim() != 1 or starts.dtype not in (torch.int64, torch.int32, torch.int16, torch.int8,
                                                         torch.uint8):
                raise ValueError("starts must be 1-D integers")
            if not self._resident:
                starts, on_device = starts.cpu(), False
        if not on_device:
            h_starts = _host_starts(starts)
            if not checked and h_starts.size:
                bad = np.flatnonzero((h_starts < 0) | (h_starts > limit))
                if bad.size:
                    raise _index_error(int(bad[0]), int(h_starts[bad[0]]), limit)
        B = int(starts.numel()) if on_device else int(h_starts.size)

        dev = self._resolve_device()
        with torch.cuda.device(dev):
            out = [torch.empty((B, T), dtype=dtype, device=dev),
                   torch.empty((B, T), dtype=dtype, device=dev) if targets else None,
                   torch.empty((B, T), dtype=torch.int64, device=dev) if positions else None,
                   torch.empty((B, T), dtype=torch.int32, device=dev) if doc_ids else None]
            if B == 0:
                return BatchResult(*out, starts if checked else None)
            sep = self._separators_on_device() if (positions or doc_ids) else None
            # what the kernel can report: a start it was not given checked, an id too wide for int32
            check = (on_device and not checked) or (dtype == torch.int32 and self._eb == 4)
            if check and self._status is None:
                self._status = torch.empty(1, dtype=torch.int64, device=dev)
            flags = (_lib.BATCH_CHECK if check else 0) | (_lib.BATCH_IGNORE if ignore_index is not None else 0)
            P = ctypes.c_void_p
            args = _lib.BatchArgs(B, T, 4 if dtype == torch.int32 else 8, flags,
                                  out[0].data_ptr(), out[1].data_ptr() if targets else None,
                                  out[2].data_ptr() if positions else None, out[3].data_ptr() if doc_ids else None,
                                  sep.data_ptr() if sep is not None and sep.numel() else None,
                                  sep.numel() if sep is not None else 0,
                                  self._sep_id if ignore_index is not None else 0,
                                  operator.index(ignore_index) if ignore_index is not None else 0,
                                  self._status.data_ptr() if check else None)
            stream = P(torch.cuda.current_stream().cuda_stream)
            L = _lib.lib()
            if self._resident:
                if on_device:
                    d_src = starts.to(device=dev, dtype=torch.int64).contiguous()
                else:
                    # not a blocking copy, which would wait for the stream; the host array is kept for a
                    # few calls, since a runtime may still read pageable memory after the call returns
                    self._host_starts.append(h_starts)
                    d_src = torch.from_numpy(h_starts).to(dev, non_blocking=True)
                rc = L.bpe_ids_batch_rows_device(P(self._ids.data_ptr()), self._n, self._eb, P(d_src.data_ptr()), None,
                                                 ctypes.byref(args), stream)
            else:
                handle, lock = _stage(dev.index)
                with lock:
                    rc = L.bpe_batch_stage_rows(handle, P(self._ids.ctypes.data), self._n, self._eb,
                                                P(h_starts.ctypes.data), ctypes.byref(args), stream)
            if rc == _lib.BPE_E_ARG:
                m = re.match(r"row (\d+) starts outside", (L.bpe_last_error() or b"").decode("utf-8", "replace"))
                if m:
                    r = int(m.group(1))
                    raise _index_error(r, int(starts[r]) if on_device else int(h_starts[r]), limit)
            _lib.check(rc, "batch")
        return BatchResult(*out, starts if checked else None)

    def _resolve_device(self):
        import torch
        if self._device is None:
            self._device = torch.device("cuda", torch.cuda.current_device())
        return self._device

    def _separators_on_device(self):
        import torch
        if self._sep_dev is None:
            self._sep_dev = torch.from_numpy(self._sep_host.view(np.int64)).to(self._resolve_device())
        return self._sep_dev


def _separator_arg(separator_id):
    if separator_id is None:
        return None
    try:
        s = operator.index(separator_id)
    except TypeError as e:
        raise ValueError("separator_id must be an integer id") from e
    if s < 0 or s >= 1 << 32:
        raise ValueError("separator_id must lie in [0, 2^32)")
    return s


def _device_arg(device):
    """None, or a cuda torch.device with its index filled in.  Does not touch the device."""
    if device is None:
        return None
    import torch
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"the batch loader runs on a cuda device, not {dev}")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def _context_arg(context_length) -> int:
    try:
        T = operator.index(context_length)
    except TypeError as e:
        raise ValueError("context_length must be an integer") from e
    if T < 1 or T >= 1 << 31:
        raise ValueError("context_length must be in [1, 2^31)")
    return T


def _host_starts(starts) -> np.ndarray:
    """Host starts (a list, an array, a CPU tensor) as a contiguous 1-D np.int64 array."""
    try:
        import torch
        if isinstance(starts, torch.Tensor):
            starts = starts.numpy()
    except ImportError:
        pass
    a = np.asarray(starts)
    if a.ndim == 1 and a.size == 0 and a.dtype.kind == "f" and not isinstance(starts, np.ndarray):
        a = a.astype(np.int64)   # an empty list
    if a.ndim != 1 or a.dtype.kind not in "iu":
        raise ValueError("starts must be 1-D integers")
    if a.dtype == np.uint64 and a.size and int(a.max()) >= 1 << 63:
        raise IndexError(f"row {int(np.argmax(a >= 1 << 63))}: start {int(a.max())} is out of range")
    return np.ascontiguousarray(a, dtype=np.int64)


def _index_error(row: int, start: int, limit: int) -> IndexError:
    return IndexError(f"row {row}: start {start} is outside [0, {limit}]")


def load_batch(dataset, batch_size, context_length, device, generator=None):
    """Drop-in for the reference's load_batch (models/util.py:37-57): (inputs, targets), int64
    [batch_size, context_length] tensors on `device`.

    The starts are drawn as the reference draws them, one torch.randint(len(dataset) -
    context_length, (batch_size,), generator=generator) on the CPU: the same values for the same
    seed, the generator left in the same state, and whatever torch.randint raises for a dataset that
    is too short.  dataset: a 1-D NumPy array or memmap of uint16, int16 (bits read as unsigned),
    uint32 or int32, served through the staging handle of `device`, or a TokenStore."""
    import torch
    start_idx = torch.randint(len(dataset) - context_length, (batch_size,), generator=generator)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"the batch loader runs on a cuda device, not {dev} (there is no CPU fallback)")
    torch.empty(0, device=dev)   # a device that is not visible raises here, as torch raises it
    dev = _device_arg(dev)
    if isinstance(dataset, TokenStore):
        store = dataset
        if store.device is not None and store.device != dev:
            raise ValueError(f"the store lives on {store.device}, not on {dev}")
        if store.device is None:
            store._device = dev
    else:
        store = TokenStore.from_array(dataset, device=dev)
    b = store.batch(start_idx, context_length, dtype=torch.int64)
    return b.inputs, b.targets
