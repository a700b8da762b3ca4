"""CPU: the inputs of tests/batch_cases.py reach what they claim.

The restated tile length equals the constexpr line of csrc/batch.hip, so a retune fails here and not
in the premise of the GPU tests; the row lengths stand on both sides of it; the alignment starts
cover every residue at both ends of the valid range; every separator placement has the property it
is named for, computed from the data alone; and the expectation helpers agree with a plain Python
loop over one row.
"""
from __future__ import annotations

import pathlib
import re

import numpy as np
import pytest

import batch_cases as C

CSRC = pathlib.Path(__file__).resolve().parent.parent / "transformer-lm_amd" / "csrc"


def test_tile_length_is_the_kernels():
    text = (CSRC / "batch.hip").read_text()
    m = re.search(r"constexpr unsigned kBatchTile = (\d+);", text)
    assert m and int(m.group(1)) == C.TILE
    m = re.search(r"constexpr unsigned kBatchThreads = (\d+);", text)
    assert m and C.TILE % int(m.group(1)) == 0


def test_row_lengths_cover_the_issue_and_the_tile():
    assert set((1, 3, 4, 5, 7, 8, 9, 255, 256, 257)) <= set(C.ROW_LENGTHS)
    assert {C.TILE - 1, C.TILE, C.TILE + 1, 3 * C.TILE} <= set(C.ROW_LENGTHS)
    assert -(-3 * C.TILE // C.TILE) == 3          # a row of exactly three tiles
    assert C.MANY_ROWS > 65535


@pytest.mark.parametrize("elem", sorted(C.ELEM))
def test_alignment_stream(elem):
    data = C.align_stream(elem)
    assert data.dtype == C.ELEM[elem] and data.size == C.N_ALIGN
    sep = np.flatnonzero(data == C.SEP)
    assert sep.size > 20 and sep[0] == 50
    if elem == "u32":
        assert int(data.max()) > 1 << 16 and int(data.max()) < 1 << 31
    for T in C.ROW_LENGTHS:
        for targets in (True, False):
            s = C.align_starts(data.size, T, targets)
            limit = data.size - T - (1 if targets else 0)
            assert s.min() == 0 and s.max() == limit
            assert set(s[:9] % 8) == set(range(8)) and set(s[-9:] % 8) == set(range(8))
            assert int(s.max()) + T + (1 if targets else 0) == data.size      # the last id is read


def _loop_row(data, sep, s, T):
    """positions and doc_ids of one row by the definition, one token at a time."""
    pos, doc = [], []
    sep = [int(p) for p in sep]
    for t in range(T):
        g = s + t
        before = [p for p in sep if p < g]
        pos.append(g - (before[-1] if before else -1) - 1)
        doc.append(sum(1 for p in sep if s <= p < g))
    return pos, doc


@pytest.mark.parametrize("name", C.PLACEMENTS)
def test_placements(name):
    data, sep, starts, T = C.placement(name)
    s = int(starts[0])
    assert np.array_equal(np.flatnonzero(data == C.SEP), sep)
    assert starts.min() >= 0 and starts.max() + T + 1 <= data.size
    assert len(set(starts.tolist())) < len(starts)                  # a duplicate row
    rel = sep - s
    inside = rel[(rel >= 0) & (rel < T)]
    if name == "row_first_and_last":
        assert inside.tolist() == [0, T - 1]
    elif name == "before_the_row":
        assert rel.tolist() == [-1]
    elif name == "after_the_row":
        assert rel.tolist() == [T]
    elif name == "none_at_all":
        assert sep.size == 0
    elif name == "far_before":
        assert sep.size == 1 and s - int(sep[0]) > 2000
    elif name == "runs_of_two_and_three":
        assert np.diff(inside).tolist().count(1) == 3 and inside.size == 5
    elif name == "separators_only":
        assert inside.size == T and rel.min() < 0 and rel.max() >= T
    elif name == "tile_last_and_first":
        assert inside.tolist() == [C.TILE - 1, C.TILE] and T > 2 * C.TILE
    elif name == "three_tiles_first_only":
        assert T == 3 * C.TILE and inside.tolist() == [5]
    elif name == "one_entry":
        assert sep.size == 1
    # the helpers against the definition, on the row the case is named for
    positions, doc_ids = C.expected_docs(sep, starts, T)
    want_pos, want_doc = _loop_row(data, sep, s, T)
    assert positions[0].tolist() == want_pos and doc_ids[0].tolist() == want_doc
    assert doc_ids[:, 0].tolist() == [0] * len(starts)
    x, y = C.expected_xy(data, starts, T)
    assert x[0].tolist() == data[s:s + T].tolist() and y[0].tolist() == data[s + 1:s + T + 1].tolist()
    ign = C.expected_ignore(x, y)
    assert np.array_equal(ign[x != C.SEP], y[x != C.SEP]) and np.all(ign[x == C.SEP] == C.IGNORE)


def test_no_separators_means_the_global_index():
    data, sep, starts, T = C.placement("none_at_all")
    positions, doc_ids = C.expected_docs(sep, starts, T)
    assert np.array_equal(positions, starts[:, None] + np.arange(T)) and not doc_ids.any()


def test_wide_stream_and_corpus():
    data, at = C.wide_stream()
    assert data.dtype == np.uint32 and int(data[at]) == 1 << 31 and int(np.delete(data, at).max()) < 1 << 31
    text = C.byte_corpus()
    assert text.count(b"<|endoftext|>") == 40 and text.endswith(b"<|endoftext|>")
