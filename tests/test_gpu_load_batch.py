"""The batch loader on the GPU: TokenStore.batch / sample and load_batch (bpe_amd.batches,
csrc/batch.hip) against NumPy on the host array.

Expected values never come from the code under test: inputs and targets are fancy-indexed slices of
the host array, positions and doc_ids come from np.searchsorted on the separator positions
(tests/batch_cases.py, checked on the CPU by tests/test_batch_cases.py).
"""
import functools
import os

import numpy as np
import pytest
import torch

import batch_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
OUT = {"i32": torch.int32, "i64": torch.int64}


def _batches():
    from bpe_amd import batches
    return batches


def _to_torch(a: np.ndarray) -> torch.Tensor:
    """The array's bits as a cuda tensor (uint16 -> int16, uint32 -> int32)."""
    signed = {2: np.int16, 4: np.int32}[a.dtype.itemsize]
    return torch.from_numpy(np.ascontiguousarray(a).view(signed).copy()).to(DEV)


@functools.lru_cache(maxsize=None)
def _align_tensor(elem):
    return _to_torch(C.align_stream(elem))


@pytest.fixture(scope="module", autouse=True)
def _drop_cached():
    yield
    _align_tensor.cache_clear()
    _batches().release_staging()


def _same(got: torch.Tensor, want: np.ndarray, dtype=None):
    assert got.is_cuda and tuple(got.shape) == want.shape, (got.shape, want.shape)
    if dtype is not None:
        assert got.dtype == dtype
    assert np.array_equal(got.cpu().numpy().astype(np.int64), want.astype(np.int64))


# ---------------------------------------------------------------------- types, lengths, alignments
@pytest.mark.parametrize("T", C.ROW_LENGTHS)
@pytest.mark.parametrize("out", sorted(OUT))
@pytest.mark.parametrize("elem", sorted(C.ELEM))
def test_rows_at_every_alignment(elem, out, T):
    """Starts at every residue modulo 8 at both ends of the valid range, on the stream itself and on
    tensor[k:] for k = 1..7 (a base pointer off the 16-byte grid), with and without targets."""
    B = _batches()
    data = C.align_stream(elem)
    whole = _align_tensor(elem)
    for k in range(8):
        store = B.TokenStore.from_tensor(whole[k:])
        host = data[k:]
        assert store.n_ids == host.size and store.dtype == C.ELEM[elem]
        for targets in (True, False):
            s = C.align_starts(host.size, T, targets)
            x, y = C.expected_xy(host, s, T)
            b = store.batch(s, T, dtype=OUT[out], targets=targets)
            _same(b.inputs, x, OUT[out])
            if targets:
                _same(b.targets, y, OUT[out])
            else:
                assert b.targets is None and y is None
            assert b.positions is None and b.doc_ids is None and b.starts is None


@pytest.mark.parametrize("T", (1, 9, 256, C.TILE + 1))
def test_starts_as_list_array_cpu_and_cuda_tensor(T):
    B = _batches()
    data = C.align_stream("u16")
    store = B.TokenStore.from_tensor(_align_tensor("u16"))
    s = C.align_starts(data.size, T, True)
    x, y = C.expected_xy(data, s, T)
    for starts in (s.tolist(), s, s.astype(np.int32), torch.from_numpy(s), torch.from_numpy(s).to(DEV),
                   torch.from_numpy(s).to(DEV, torch.int32)):
        b = store.batch(starts, T)
        _same(b.inputs, x, torch.int64)
        _same(b.targets, y, torch.int64)


def test_row_sets():
    B = _batches()
    data = C.align_stream("u16")
    store = B.TokenStore.from_tensor(_align_tensor("u16"))
    # duplicates and overlaps
    s = np.asarray([100, 100, 101, 99, 100, 130, 100], dtype=np.int64)
    x, y = C.expected_xy(data, s, 64)
    b = store.batch(s, 64)
    _same(b.inputs, x)
    _same(b.targets, y)
    # one row, no rows
    b = store.batch([17], 33)
    _same(b.inputs, data[None, 17:50])
    _same(b.targets, data[None, 18:51])
    for starts in ([], np.zeros(0, dtype=np.int64), torch.zeros(0, dtype=torch.int64, device=DEV)):
        b = store.batch(starts, 12, dtype=torch.int32)
        assert tuple(b.inputs.shape) == (0, 12) == tuple(b.targets.shape) and b.inputs.dtype == torch.int32
        assert b.inputs.is_cuda
    # more rows than a grid dimension of 65 535
    s = np.random.default_rng(3).integers(0, data.size - 2, C.MANY_ROWS)
    s[-1] = data.size - 2
    b = store.batch(torch.from_numpy(s).to(DEV), 1)
    x, y = C.expected_xy(data, s, 1)
    _same(b.inputs, x)
    _same(b.targets, y)


# ---------------------------------------------------------------------- documents
@pytest.mark.parametrize("name", C.PLACEMENTS)
def test_separator_placements(name):
    B = _batches()
    data, sep, starts, T = C.placement(name)
    ids = _to_torch(data)
    by_id = B.TokenStore.from_tensor(ids, separator_id=C.SEP)      # positions found by the ids_find kernel
    assert by_id.n_docs == sep.size and by_id.separator_positions.tolist() == sep.tolist()
    x, y = C.expected_xy(data, starts, T)
    positions, doc_ids = C.expected_docs(sep, starts, T)
    for out in sorted(OUT):
        b = by_id.batch(starts, T, dtype=OUT[out], positions=True, doc_ids=True)
        _same(b.inputs, x, OUT[out])
        _same(b.targets, y, OUT[out])
        _same(b.positions, positions, torch.int64)
        _same(b.doc_ids, doc_ids, torch.int32)
        # ignore_index: where the input is the separator, and nowhere else
        b = by_id.batch(torch.from_numpy(starts).to(DEV), T, dtype=OUT[out], doc_ids=True, ignore_index=C.IGNORE)
        got = b.targets.cpu().numpy()
        want = C.expected_ignore(x, y)
        assert np.array_equal(got, want)
        assert np.array_equal(got[x != C.SEP], y[x != C.SEP]) and np.all(got[x == C.SEP] == C.IGNORE)
        _same(b.inputs, x)
        _same(b.doc_ids, doc_ids, torch.int32)
        assert b.positions is None
    # one output without the other, without targets
    b = by_id.batch(starts, T, targets=False, positions=True)
    _same(b.positions, positions)
    assert b.targets is None and b.doc_ids is None


def test_document_outputs_on_an_offset_store_and_odd_lengths():
    """tensor[k:] with its own separators, T off every vector width: the tile's output alignment
    differs from row to row."""
    B = _batches()
    data = C.align_stream("u32")
    whole = _align_tensor("u32")
    for k, T in ((1, 257), (3, C.TILE + 1), (6, 5)):
        host = data[k:]
        sep = np.flatnonzero(host == C.SEP)
        store = B.TokenStore.from_tensor(whole[k:], separator_id=C.SEP)
        s = C.align_starts(host.size, T, True)
        positions, doc_ids = C.expected_docs(sep, s, T)
        x, y = C.expected_xy(host, s, T)
        b = store.batch(s, T, dtype=torch.int32, positions=True, doc_ids=True, ignore_index=C.IGNORE)
        _same(b.positions, positions)
        _same(b.doc_ids, doc_ids)
        _same(b.inputs, x)
        _same(b.targets, C.expected_ignore(x, y))


# ---------------------------------------------------------------------- the checks of the kernel
def test_int32_limit():
    B = _batches()
    data, at = C.wide_stream()
    store = B.TokenStore.from_tensor(_to_torch(data))
    with pytest.raises(RuntimeError, match=str(1 << 31)):
        store.batch([at - 5, 0], 16, dtype=torch.int32)
    with pytest.raises(RuntimeError, match=str(1 << 31)):       # seen by the target alone
        store.batch([at - 16], 16, dtype=torch.int32)
    b = store.batch([0, at + 1, at - 17], 16, dtype=torch.int32)   # the id lies outside every row
    x, y = C.expected_xy(data, [0, at + 1, at - 17], 16)
    _same(b.inputs, x)
    _same(b.targets, y)
    b = store.batch([at - 16], 16, dtype=torch.int32, targets=False)
    _same(b.inputs, C.expected_xy(data, [at - 16], 16)[0])
    b = store.batch([at - 5], 16)                                  # int64 holds it
    x, y = C.expected_xy(data, [at - 5], 16)
    _same(b.inputs, x, torch.int64)
    _same(b.targets, y, torch.int64)
    assert int(b.inputs[0, 5]) == 1 << 31


def test_cuda_starts_out_of_range():
    B = _batches()
    data = C.align_stream("u16")
    store = B.TokenStore.from_tensor(_align_tensor("u16"))
    n, T = data.size, 40
    starts = torch.tensor([5, n - T - 1, n - T, 7, -1], device=DEV)
    with pytest.raises(IndexError, match=rf"row 2: start {n - T} is outside \[0, {n - T - 1}\]"):
        store.batch(starts, T)
    b = store.batch(starts[:4], T, targets=False)                 # n - T is valid without targets
    _same(b.inputs, C.expected_xy(data, [5, n - T - 1, n - T, 7], T)[0])
    with pytest.raises(IndexError, match=r"row 4: start -1 is outside"):
        store.batch(starts, T, targets=False)
    with pytest.raises(IndexError, match=r"row 0: start -1 is outside"):
        store.batch(torch.tensor([-1, n], device=DEV), T)
    # a good call after a refused one
    b = store.batch(starts[:2], T)
    _same(b.inputs, C.expected_xy(data, [5, n - T - 1], T)[0])


# ---------------------------------------------------------------------- host mode
def test_host_mode_equals_resident_mode(tmp_path):
    B = _batches()
    data, sep, _, _ = C.placement("runs_of_two_and_three")
    path, idx = tmp_path / "train.bin", tmp_path / "train.idx"
    data.tofile(path)
    sep.astype(np.uint64).tofile(idx)
    resident = B.TokenStore.from_file(path, np.uint16, index_path=idx, separator_id=C.SEP)
    assert resident.resident and resident.n_docs == sep.size and resident.device_bytes == data.nbytes + 8 * sep.size
    hosts = [B.TokenStore.from_array(data.copy(), index_path=idx, separator_id=C.SEP),
             B.TokenStore.from_array(np.memmap(path, dtype=np.uint16, mode="r"), index_path=idx, separator_id=C.SEP),
             B.TokenStore.from_file(path, np.uint16, index_path=idx, separator_id=C.SEP, resident=False)]
    rng = np.random.default_rng(9)
    T = 300
    s1 = rng.integers(0, data.size - T - 1, 37)
    s1[:3] = (0, data.size - T - 1, 5000)
    s2 = rng.integers(0, data.size - T - 1, 5)
    for host in hosts:
        assert not host.resident and host.device_bytes == 0
        # two calls back to back, nothing in between: the second must not overwrite what the first reads
        a = host.batch(s1, T, positions=True, doc_ids=True, ignore_index=C.IGNORE)
        b = host.batch(s2, T, dtype=torch.int32, positions=True, doc_ids=True)
        for got, s, kw in ((a, s1, {"ignore_index": C.IGNORE}), (b, s2, {"dtype": torch.int32})):
            want = resident.batch(s, T, positions=True, doc_ids=True, **kw)
            x, y = C.expected_xy(data, s, T)
            _same(got.inputs, x)
            _same(got.targets, C.expected_ignore(x, y) if kw.get("ignore_index") else y)
            for f in ("inputs", "targets", "positions", "doc_ids"):
                assert torch.equal(getattr(got, f), getattr(want, f)), f
            positions, doc_ids = C.expected_docs(sep, s, T)
            _same(got.positions, positions)
            _same(got.doc_ids, doc_ids)
        assert host.device_bytes == 8 * sep.size
    resident.close()


def test_staging_grows_and_is_reused():
    B = _batches()
    data = C.filler(300_000, 41)
    store = B.TokenStore.from_array(data)
    rng = np.random.default_rng(2)
    calls = []
    # large, small, larger, small, large: 1.6 MB of rows are copied by three threads, 4.8 MB by eight
    for rows, T in ((2000, 400), (2, 3), (6000, 400), (1, 1), (2000, 400)):
        s = rng.integers(0, data.size - T - 1, rows)
        calls.append((s, T, store.batch(s, T)))
    for s, T, got in calls:
        x, y = C.expected_xy(data, s, T)
        _same(got.inputs, x, torch.int64)
        _same(got.targets, y, torch.int64)
    with pytest.raises(IndexError, match="row 1: start 299999"):
        store.batch([0, 299_999], 4)
    b = store.batch(torch.tensor([3, 4], device=DEV), 4, targets=False)        # cuda starts come to the host
    _same(b.inputs, C.expected_xy(data, [3, 4], 4)[0])


# ---------------------------------------------------------------------- files written by encode_files
def test_from_file_with_the_index_encode_files_writes(tmp_path):
    import bpe_amd
    B = _batches()
    vocab = {i: bytes([i]) for i in range(256)}
    vocab[256] = b"<|endoftext|>"
    tok = bpe_amd.Tokenizer(vocab, [], ["<|endoftext|>"])
    text = C.byte_corpus()
    src, out, idx = tmp_path / "c.txt", tmp_path / "train.bin", tmp_path / "train.idx"
    src.write_bytes(text)
    info = bpe_amd.encode_files(tok, [src], out, separator="<|endoftext|>", index_path=idx)
    del tok
    n_sep = text.count(b"<|endoftext|>")
    data = np.fromfile(out, dtype=np.uint16)
    sep = np.flatnonzero(data == 256)
    assert info["n_separators"] == n_sep == sep.size
    both = B.TokenStore.from_file(out, np.uint16, index_path=idx, separator_id=256)
    by_index = B.TokenStore.from_file(out, np.uint16, index_path=idx)
    by_id = B.TokenStore.from_file(out, np.uint16, separator_id=256)
    for st in (both, by_index, by_id):
        assert st.n_docs == n_sep and st.n_ids == data.size and st.dtype == np.uint16
        assert st.separator_positions.tolist() == sep.tolist()
    s = np.asarray([0, 1, int(sep[3]), int(sep[3]) + 1, data.size - 65], dtype=np.int64)
    positions, doc_ids = C.expected_docs(sep, s, 64)
    for st in (by_index, by_id):
        b = st.batch(s, 64, positions=True, doc_ids=True)
        _same(b.inputs, C.expected_xy(data, s, 64)[0])
        _same(b.positions, positions)
        _same(b.doc_ids, doc_ids)
    # one entry of the index changed: refused at open by a resident store
    wrong = np.fromfile(idx, dtype=np.uint64)
    wrong[int(np.flatnonzero(np.diff(sep) > 1)[0]) + 1] -= 1       # still ascending: only the device can tell
    bad = tmp_path / "wrong.idx"
    wrong.tofile(bad)
    with pytest.raises(ValueError, match="wrong.idx"):
        B.TokenStore.from_file(out, np.uint16, index_path=bad, separator_id=256)
    with pytest.raises(ValueError):
        B.TokenStore.from_file(out, np.uint16, index_path=idx, separator_id=97)
    assert B.TokenStore.from_file(out, np.uint16, index_path=bad, separator_id=256, resident=False).n_docs == n_sep


# ---------------------------------------------------------------------- the drop-in and sample
@pytest.mark.parametrize("seed", range(5))
def test_load_batch_draws_as_the_reference_does(seed, tmp_path):
    B = _batches()
    data = C.align_stream("u16")
    path = tmp_path / "tokens.bin"
    data.tofile(path)
    mm = np.memmap(path, dtype=np.uint16, mode="r")
    store = B.TokenStore.from_tensor(_align_tensor("u16"))
    bs, T = 16, 100 + seed
    for dataset in (mm, store, data.view(np.int16)):
        g, h = torch.Generator().manual_seed(seed), torch.Generator().manual_seed(seed)
        x, y = B.load_batch(dataset, bs, T, DEV, generator=g)
        s = torch.randint(len(data) - T, (bs,), generator=h).numpy()
        want_x, want_y = C.expected_xy(data, s, T)
        _same(x, want_x, torch.int64)
        _same(y, want_y, torch.int64)
        assert torch.equal(torch.randint(1 << 40, (3,), generator=g), torch.randint(1 << 40, (3,), generator=h))
    x, y = B.load_batch(mm, 2, 7, torch.device("cuda:0"))       # the global generator, a torch.device
    assert x.dtype == torch.int64 and x.device == torch.device("cuda:0") and tuple(y.shape) == (2, 7)
    with pytest.raises(RuntimeError):
        B.load_batch(mm, 2, 7, f"cuda:{torch.cuda.device_count()}")


@pytest.mark.parametrize("targets", (True, False))
def test_sample(targets):
    B = _batches()
    data, sep, _, _ = C.placement("runs_of_two_and_three")
    ids = _to_torch(data)
    resident = B.TokenStore.from_tensor(ids, separator_id=C.SEP)
    host = B.TokenStore.from_array(data)
    T = data.size - 40                   # few valid starts: the ends of the range are drawn
    g = torch.Generator(device=DEV).manual_seed(1)
    for store, kw in ((resident, {"generator": g, "positions": True, "doc_ids": True}), (host, {})):
        b = store.sample(64, T, targets=targets, **kw)
        s = b.starts.cpu().numpy()
        assert b.starts.is_cuda == store.resident and s.shape == (64,)
        limit = data.size - T - (1 if targets else 0)
        assert s.min() >= 0 and s.max() <= limit and len(set(s.tolist())) > 10
        x, y = C.expected_xy(data, s, T)
        _same(b.inputs, x)
        if targets:
            _same(b.targets, y)
        else:
            assert b.targets is None
        if "positions" in kw:
            positions, doc_ids = C.expected_docs(sep, s, T)
            _same(b.positions, positions)
            _same(b.doc_ids, doc_ids)
    assert tuple(resident.sample(0, 8).inputs.shape) == (0, 8)
