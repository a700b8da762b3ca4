"""bench.py's command line (no GPU): a plain run keeps only the timed steps, --full restores the
side legs, and --dump-outputs writes the step's (vocab, merges) as float32 arrays that give the
result back exactly."""
from __future__ import annotations

import sys

import numpy as np

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_has_no_side_legs(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert a.no_device_resident and a.no_encode and a.no_cpu_baseline


def test_no_file_keeps_the_resident_leg_as_the_timed_path(monkeypatch):
    a = _parse(monkeypatch, "--no-file")
    assert not a.no_device_resident and a.no_encode and a.no_cpu_baseline


def test_full_runs_every_leg_unless_switched_off(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert not (a.no_device_resident or a.no_encode or a.no_cpu_baseline)
    a = _parse(monkeypatch, "--full", "--no-encode")
    assert a.no_encode and not a.no_cpu_baseline


def test_dump_outputs_round_trip(tmp_path):
    vocab = {0: b"<|endoftext|>", 1: b"a", 2: b"\xff", 3: b"a\xff", 4: b""}
    merges = [(b"a", b"\xff"), (b"a\xff", b"a")]
    bench.dump_outputs(tmp_path / "out", vocab, merges)
    got = {p.stem: np.load(p) for p in (tmp_path / "out").glob("*.npy")}
    assert sorted(got) == ["merges_bytes", "merges_lens", "vocab_bytes", "vocab_lens"]
    assert all(a.dtype == np.float32 for a in got.values())
    raw = bytes(got["vocab_bytes"].astype(np.uint8))
    ends = np.cumsum(got["vocab_lens"]).astype(int)
    assert [raw[e - int(n):e] for e, n in zip(ends, got["vocab_lens"])] == [vocab[i] for i in range(5)]
    assert got["merges_lens"].tolist() == [[1, 1], [2, 1]]
    assert bytes(got["merges_bytes"].astype(np.uint8)) == b"a\xffa\xffa"
