"""Inputs of the batch loader's tests (tests/test_gpu_load_batch.py) and their expected values, by
NumPy on the host array alone; tests/test_batch_cases.py shows that they reach what they claim.

    x = data[s[:, None] + arange(T)],  y one further
    sep = flatnonzero(data == SEP)
    positions, doc_ids from searchsorted(sep, g, "left")
"""
from __future__ import annotations

import functools

import numpy as np

TILE = 1024          # csrc/batch.hip: kBatchTile (held against the source by test_batch_cases.py)
SEP = 7              # the separator id of the synthetic streams; fillers never use it
IGNORE = -100
ROW_LENGTHS = (1, 3, 4, 5, 7, 8, 9, 255, 256, 257, TILE - 1, TILE, TILE + 1, 3 * TILE)
ELEM = {"u16": np.uint16, "u32": np.uint32}
N_ALIGN = 3 * TILE + 37                  # the alignment stream: the longest row has 36 valid starts; odd
MANY_ROWS = 70_000                       # above a grid dimension of 65 535


def filler(n: int, seed: int, dtype=np.uint16) -> np.ndarray:
    """n ids in [8, 60000): none of them SEP."""
    return np.random.default_rng(seed).integers(8, 60000, n).astype(dtype)


@functools.lru_cache(maxsize=None)
def align_stream(elem: str) -> np.ndarray:
    """Ids with a separator every 97 ids; uint32 ids carry bits above 16 (below 2^31)."""
    data = filler(N_ALIGN, 11, ELEM[elem])
    if elem == "u32":
        data = data | (np.arange(N_ALIGN, dtype=np.uint32) % 5 << 27)
    data[50::97] = SEP
    data.setflags(write=False)
    return data


def align_starts(n: int, T: int, targets: bool) -> np.ndarray:
    """Start 0 and the next 8, and the last valid start and the 8 before it: every residue modulo 8
    at both ends of the range, duplicates where the two groups meet."""
    limit = n - T - (1 if targets else 0)
    lo = np.arange(0, min(9, limit + 1))
    hi = np.arange(max(0, limit - 8), limit + 1)
    return np.concatenate([lo, hi]).astype(np.int64)


def expected_xy(data: np.ndarray, starts, T: int):
    """(inputs, targets) as int64; targets is None where a row has no id one further."""
    s = np.asarray(starts, dtype=np.int64)
    idx = s[:, None] + np.arange(T, dtype=np.int64)[None, :]
    x = data[idx].astype(np.int64)
    y = data[idx + 1].astype(np.int64) if (s.size == 0 or int(s.max()) + T < data.size) else None
    return x, y


def expected_docs(sep, starts, T: int):
    """(positions int64, doc_ids int32) from the sorted separator positions."""
    sep = np.asarray(sep, dtype=np.int64)
    s = np.asarray(starts, dtype=np.int64)
    g = s[:, None] + np.arange(T, dtype=np.int64)[None, :]
    k = np.searchsorted(sep, g, "left")                       # separators below g
    last = np.where(k > 0, sep[np.maximum(k, 1) - 1] if sep.size else -1, -1)
    positions = g - last - 1
    doc_ids = k - np.searchsorted(sep, s, "left")[:, None]
    return positions.astype(np.int64), doc_ids.astype(np.int32)


def expected_ignore(x: np.ndarray, y: np.ndarray, sep_id: int = SEP, ignore: int = IGNORE) -> np.ndarray:
    return np.where(x == sep_id, ignore, y)


# ---------------------------------------------------------------------- separator placements
# name -> (T, start s, separator positions as a function of (s, T))
N_SEP_STREAM = 24_000
_PLACEMENTS = {
    "row_first_and_last": (64, 5000, lambda s, T: [s, s + T - 1]),
    "before_the_row": (64, 5000, lambda s, T: [s - 1]),
    "after_the_row": (64, 5000, lambda s, T: [s + T]),
    "none_at_all": (64, 5000, lambda s, T: []),
    "far_before": (64, 9000, lambda s, T: [17]),
    "runs_of_two_and_three": (64, 5000, lambda s, T: [s + 10, s + 11, s + 20, s + 21, s + 22]),
    "separators_only": (64, 5000, lambda s, T: list(range(s - 2, s + T + 2))),
    "tile_last_and_first": (2 * TILE + 100, 3001, lambda s, T: [s + TILE - 1, s + TILE]),
    "three_tiles_first_only": (3 * TILE, 2000, lambda s, T: [s + 5]),
    "one_entry": (64, 5000, lambda s, T: [s + 3]),
}
PLACEMENTS = tuple(_PLACEMENTS)


@functools.lru_cache(maxsize=None)
def placement(name: str):
    """-> (data uint16, sep positions int64, starts int64, T): the row the case is named for at
    starts[0], then overlapping neighbours and a duplicate of it."""
    T, s, where = _PLACEMENTS[name]
    data = filler(N_SEP_STREAM, 23)
    sep = np.asarray(sorted(where(s, T)), dtype=np.int64)
    data[sep] = SEP
    data.setflags(write=False)
    starts = np.asarray([s, s + 1, s - 3, s + T // 2, s], dtype=np.int64)
    return data, sep, starts, T


# ---------------------------------------------------------------------- the int32 limit
def wide_stream():
    """uint32 ids with one id of 2^31 at position 300 -> (data, position)."""
    data = filler(1000, 31, np.uint32)
    data[300] = 1 << 31
    data.setflags(write=False)
    return data, 300


def byte_corpus() -> bytes:
    """A small text with separators for the encode_files round trip (byte-level tokenizer)."""
    rng = np.random.default_rng(5)
    docs = []
    for i in range(40):
        docs.append(bytes(rng.integers(97, 123, int(rng.integers(0, 300))).astype(np.uint8)))
    return b"<|endoftext|>".join(docs) + b"<|endoftext|>"
