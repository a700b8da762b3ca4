"""CPU: what the batch loader (bpe_amd.batches) refuses before the device is touched -- every
ValueError and IndexError of TokenStore.batch / sample and of the constructors, the host range check,
the size check of from_file -- and the argument checks of the C entry points that need no device.
None of these tests needs a GPU: a check that reached the device would raise RuntimeError here.
"""
import ctypes

import numpy as np
import pytest
import torch

import bpe_amd
from bpe_amd import _lib, batches
from bpe_amd.batches import TokenStore

NEW = ["bpe_ids_batch_rows_device", "bpe_batch_stage_create", "bpe_batch_stage_rows", "bpe_batch_stage_free"]


def _store(n=100, dtype=np.uint16, **kw):
    return TokenStore.from_array(np.arange(n).astype(dtype), **kw)


def _index_file(tmp_path, positions, name="t.idx"):
    p = tmp_path / name
    np.asarray(positions, dtype=np.uint64).tofile(p)
    return p


def test_symbols_and_lazy_names():
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(L, name)
    assert L.bpe_abi_version() == 2
    assert bpe_amd.load_batch is batches.load_batch and bpe_amd.TokenStore is TokenStore


def test_properties_of_a_host_store(tmp_path):
    st = _store(100, np.int16)
    assert (st.n_ids, len(st), st.dtype, st.n_docs, st.device_bytes, st.resident) == (100, 100, np.uint16, None, 0, False)
    st = _store(100, np.int32, index_path=_index_file(tmp_path, [3, 50, 99]), separator_id=5)
    assert st.dtype == np.uint32 and st.n_docs == 3 and st.separator_id == 5
    assert st.separator_positions.tolist() == [3, 50, 99]
    with _store() as st2:
        pass
    with pytest.raises(ValueError, match="closed"):
        st2.batch([0], 4)


@pytest.mark.parametrize("bad", [np.arange(10, dtype=np.int64), np.arange(10, dtype=np.uint8),
                                 np.zeros((2, 5), dtype=np.uint16), np.arange(20, dtype=np.uint16)[::2],
                                 [1, 2, 3], np.arange(10, dtype=np.float32)])
def test_from_array_refuses(bad):
    with pytest.raises(ValueError):
        TokenStore.from_array(bad)


def test_from_tensor_refuses_what_is_not_a_cuda_id_tensor():
    for bad in (torch.zeros(8, dtype=torch.int32), np.zeros(8, dtype=np.uint16), [1, 2]):
        with pytest.raises(ValueError):
            TokenStore.from_tensor(bad)


def test_from_file_size_check(tmp_path):
    p = tmp_path / "odd.bin"
    p.write_bytes(b"\x01\x00\x02")
    for resident in (True, False):
        with pytest.raises(ValueError, match="whole number"):
            TokenStore.from_file(p, np.uint16, resident=resident)
    p.write_bytes(b"\x01\x00\x02\x00\x03\x00")
    with pytest.raises(ValueError, match="whole number"):
        TokenStore.from_file(p, np.uint32, resident=False)
    with pytest.raises(ValueError):
        TokenStore.from_file(p, np.float32)
    with pytest.raises(ValueError):
        TokenStore.from_file(p, np.uint16, resident=False, separator_id=-1)
    with pytest.raises(ValueError):
        TokenStore.from_file(p, np.uint16, resident=False, device="cpu")
    with pytest.raises(FileNotFoundError):
        TokenStore.from_file(tmp_path / "missing.bin", np.uint16)
    st = TokenStore.from_file(p, np.uint16, resident=False)
    assert st.n_ids == 3 and not st.resident and st.n_docs is None


def test_index_file_checks(tmp_path):
    p = tmp_path / "t.bin"
    np.arange(50, dtype=np.uint16).tofile(p)
    bad = tmp_path / "bad.idx"
    bad.write_bytes(b"\0" * 12)
    with pytest.raises(ValueError, match="uint64"):
        TokenStore.from_file(p, np.uint16, index_path=bad, resident=False)
    for positions in ([5, 5], [9, 3], [50]):
        with pytest.raises(ValueError, match="ascending"):
            TokenStore.from_file(p, np.uint16, index_path=_index_file(tmp_path, positions), resident=False)
    st = TokenStore.from_file(p, np.uint16, index_path=_index_file(tmp_path, []), resident=False)
    assert st.n_docs == 0


def test_batch_refuses_before_the_device(tmp_path):
    st = _store(100)
    for T in (0, -1, 1 << 31, 2.5, None):
        with pytest.raises(ValueError, match="context_length"):
            st.batch([0], T)
    for dt in (torch.int16, torch.float32, torch.uint8, np.int64):
        with pytest.raises(ValueError, match="dtype"):
            st.batch([0], 4, dtype=dt)
    for kw in ({"positions": True}, {"doc_ids": True}):
        with pytest.raises(ValueError, match="separator positions"):
            st.batch([0], 4, **kw)
        with pytest.raises(ValueError, match="separator positions"):
            st.sample(2, 4, **kw)
    with pytest.raises(ValueError, match="separator_id"):
        st.batch([0], 4, ignore_index=-100)
    sid = _store(100, separator_id=5)
    with pytest.raises(ValueError, match="targets"):
        sid.batch([0], 4, targets=False, ignore_index=-100)
    with pytest.raises(ValueError, match="fit"):
        sid.batch([0], 4, dtype=torch.int32, ignore_index=1 << 31)
    for starts in ([[0, 1]], np.zeros((2, 2), dtype=np.int64), [0.5], np.array([1.0]), torch.tensor([1.5]),
                   torch.zeros((1, 1), dtype=torch.int64), "ab", [True, False]):
        with pytest.raises(ValueError, match="starts"):
            st.batch(starts, 4)
    with pytest.raises(ValueError):
        st.sample(-1, 4)
    # an index alone serves positions; it does not serve ignore_index
    idx = _store(100, index_path=_index_file(tmp_path, [10]))
    with pytest.raises(ValueError, match="separator_id"):
        idx.batch([0], 4, positions=True, ignore_index=-100)


@pytest.mark.parametrize("make", [list, np.asarray, torch.tensor, lambda s: np.asarray(s, dtype=np.int32)])
def test_host_range_check(make):
    st = _store(100)
    # the last valid start is n - T - 1 with targets, n - T without
    with pytest.raises(IndexError, match=r"row 2: start 90 is outside \[0, 89\]"):
        st.batch(make([0, 89, 90, 91]), 10)
    with pytest.raises(IndexError, match=r"row 1: start 91 is outside \[0, 90\]"):
        st.batch(make([90, 91]), 10, targets=False)
    with pytest.raises(IndexError, match=r"row 0: start -1 is outside"):
        st.batch(make([-1, 500]), 10)
    with pytest.raises(IndexError, match=r"row 0: start 0 is outside \[0, -1\]"):
        st.batch(make([0]), 100)


def test_sample_and_load_batch_raise_as_randint_for_a_short_dataset():
    st = _store(10)
    with pytest.raises(RuntimeError) as a:
        torch.randint(0, (4,))
    with pytest.raises(RuntimeError) as b:
        st.sample(4, 10)
    with pytest.raises(RuntimeError) as c:
        batches.load_batch(np.arange(10, dtype=np.uint16), 4, 10, "cuda")
    assert str(a.value).splitlines()[0] == str(b.value).splitlines()[0] == str(c.value).splitlines()[0]
    with pytest.raises(ValueError, match="cuda"):
        batches.load_batch(np.arange(100, dtype=np.uint16), 4, 10, "cpu")


def test_c_entry_argument_checks():
    L = _lib.lib()
    A = _lib.BatchArgs

    def rc(n_rows=0, row_len=8, out=8, flags=0, elem=2, **kw):
        a = A(n_rows, row_len, out, flags, None, None, None, None, None, 0, 0, kw.get("ignore", 0), kw.get("status"))
        return L.bpe_ids_batch_rows_device(None, 0, elem, None, None, ctypes.byref(a), None)

    assert rc() == 0                                           # no rows
    assert rc(elem=8) == _lib.BPE_E_ARG and rc(elem=1) == _lib.BPE_E_ARG
    assert rc(out=2) == _lib.BPE_E_ARG
    assert rc(row_len=0) == _lib.BPE_E_ARG
    assert rc(flags=4) == _lib.BPE_E_ARG
    assert rc(flags=_lib.BATCH_CHECK) == _lib.BPE_E_ARG         # no status word
    assert rc(flags=_lib.BATCH_IGNORE) == _lib.BPE_E_ARG        # no targets
    assert rc(n_rows=1) == _lib.BPE_E_ARG                       # NULL arrays
    assert L.bpe_ids_batch_rows_device(None, 0, 2, None, None, None, None) == _lib.BPE_E_ARG
    assert b"NULL" in L.bpe_last_error()
    assert L.bpe_batch_stage_rows(None, None, 0, 2, None, None, None) == _lib.BPE_E_ARG
    L.bpe_batch_stage_free(None)
