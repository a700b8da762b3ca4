"""GPU: Tokenizer.encode with sparse and large vocab ids (csrc/encode.hip), against two
expectations per case and id map: the C oracle on the remapped vocab, and the map applied in plain
Python to the oracle's ids for the dense vocab.  The inputs are those of tests/vocab_id_cases.py;
tests/test_vocab_id_cases.py shows on the CPU that they hold words of every population (one byte,
vocab entry of 2..16 bytes, other word of 2..16 bytes, 17 bytes and more) and id count, and that
the edge and straddle maps put an id at or above each inline threshold (2^31, 2^20, 2^15) in
every position.

  every case x map    encode, both expectations
  run-time paths      the constructed case under top, scatter and edge(2^20) on every knob set of
                      test_gpu_encode.py's test_encode_resolution_paths
  batch forms         about 40 documents cut at arbitrary characters: encode_batch, encode_batch_np,
                      padded int64 rows, padded int32 rows where every id fits
  int32 rows          a kept id >= 2^31 fails with BPE_E_LIMIT naming the smallest such id, through
                      encode_batch_padded and bpe_ids_pack_rows_device; one truncated away does not
  two ranks           in-process ranks keep the ids of the stored vocab
  encode_file         uint16 ids of a map that fits
  decode              round trip below the decoder's 2^28; above it the documented BPE_E_LIMIT
  create              a vocab id of 2^32 or -1 is BPE_E_ARG

Before the fix that came with these tests the int32 rows held negative numbers for ids from 2^31
on and the call returned 0: test_padded_int32_refuses_wide_ids, test_pack_rows_int32_direct and
test_padded_int32_wide_id_truncated_away failed, the other 60 passed.

Measured on an MI355X: the 66 tests take 3.2 s together; the slowest is the first, which loads
the library (1.6 s of set-up); of the rest test_encode[natural-dense] takes 0.19 s with its
oracle runs, every other 0.12 s or less.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

import vocab_id_cases as V
from oracle import oracle
from test_gpu_encode import RESOLUTION_KNOBS
from test_gpu_encode_batch import _pad_want

pytestmark = pytest.mark.gpu

bpe_amd = pytest.importorskip("bpe_amd")
from bpe_amd import _lib  # noqa: E402

N_DOCS = 40


@pytest.fixture(scope="module", autouse=True)
def _device():
    _lib.require_device()


@functools.lru_cache(maxsize=None)
def _dense(case_name):
    c = V.CASES[case_name]()
    return oracle.encode(c.vocab, c.merges, c.specials, c.text)


@functools.lru_cache(maxsize=None)
def _map(case_name, map_name):
    return V.id_map(map_name, V.CASES[case_name]())


@functools.lru_cache(maxsize=None)
def _want(case_name, map_name):
    """(the oracle on the remapped vocab, the map over the oracle's dense ids)"""
    c, f = V.CASES[case_name](), _map(case_name, map_name)
    return (oracle.encode(V.remap(c, f), c.merges, c.specials, c.text), [f[i] for i in _dense(case_name)])


def _new_tok(case_name, map_name):
    c = V.CASES[case_name]()
    return bpe_amd.Tokenizer(V.remap(c, _map(case_name, map_name)), list(c.merges), list(c.specials))


@functools.lru_cache(maxsize=None)
def _tok(case_name, map_name):
    return _new_tok(case_name, map_name)


@functools.lru_cache(maxsize=None)
def _docs(case_name):
    return tuple(V.cut_documents(V.CASES[case_name]().text, N_DOCS, 11))


@functools.lru_cache(maxsize=None)
def _want_docs(case_name, map_name):
    """per document: (oracle on the remapped vocab, the map over the oracle's dense ids)"""
    c, f = V.CASES[case_name](), _map(case_name, map_name)
    vocab = V.remap(c, f)
    return ([oracle.encode(vocab, c.merges, c.specials, d) for d in _docs(case_name)],
            [[f[i] for i in oracle.encode(c.vocab, c.merges, c.specials, d)] for d in _docs(case_name)])


def _first_difference(got, want):
    k = next((j for j, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return f"{len(got)} ids against {len(want)}, first difference at {k}: {got[k:k + 6]} against {want[k:k + 6]}"


def _check(got, case_name, map_name):
    by_oracle, by_map = _want(case_name, map_name)
    assert by_oracle == by_map
    if got != by_map:
        pytest.fail(_first_difference(got, by_map))


@pytest.mark.parametrize("case_name,map_name", V.all_case_maps())
def test_encode(case_name, map_name):
    _check(_tok(case_name, map_name).encode(V.CASES[case_name]().text), case_name, map_name)


@pytest.mark.parametrize("knobs", RESOLUTION_KNOBS, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()))
@pytest.mark.parametrize("map_name", ["top", "scatter", f"edge:{V.T3}"])
def test_encode_resolution_paths(map_name, knobs, monkeypatch):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    tok = _new_tok("constructed", map_name)
    _check(tok.encode(V.constructed().text), "constructed", map_name)


# ---------------------------------------------------------------------- batch forms
BATCH = [(c, m) for c in V.CASES for m in ("top", f"edge:{V.T4}") if m in V.MAPS[c]]


@pytest.mark.parametrize("case_name,map_name", BATCH)
def test_encode_batch(case_name, map_name):
    tok, docs = _tok(case_name, map_name), list(_docs(case_name))
    by_oracle, by_map = _want_docs(case_name, map_name)
    assert by_oracle == by_map
    assert tok.encode_batch(docs) == by_map
    ids, offsets = tok.encode_batch_np(docs)
    assert ids.dtype == np.uint32 and offsets.tolist() == np.cumsum([0] + [len(r) for r in by_map]).tolist()
    assert ids.tolist() == [i for r in by_map for i in r]


def _check_padded(tok, docs, rows, dtype):
    import torch
    longest = max(map(len, rows))
    flat = np.array([i for r in rows for i in r], dtype=np.int64)
    offsets = np.cumsum([0] + [len(r) for r in rows])
    for T, truncation, padding_side in ((None, "right", "right"), (longest // 2 + 1, "left", "left"),
                                        (longest // 2, "right", "left")):
        got, lengths = tok.encode_batch_padded(docs, T, pad_id=-1, truncation=truncation, padding_side=padding_side,
                                               dtype=dtype)
        want, wlen = _pad_want(flat, offsets, longest if T is None else T, -1, truncation, padding_side,
                               np.int32 if dtype == torch.int32 else np.int64)
        assert got.dtype == dtype and np.array_equal(got.cpu().numpy(), want)
        assert np.array_equal(lengths.cpu().numpy(), wlen)


@pytest.mark.parametrize("case_name,map_name", BATCH)
def test_padded_int64(case_name, map_name):
    import torch
    _check_padded(_tok(case_name, map_name), list(_docs(case_name)), _want_docs(case_name, map_name)[1], torch.int64)


@pytest.mark.parametrize("case_name,map_name", [("constructed", f"edge:{V.T4}"), ("natural", f"straddle:{V.T3}"),
                                                ("constructed", f"straddle:{V.DIRECT}")])
def test_padded_int32_ids_that_fit(case_name, map_name):
    """maps whose ids are all below 2^31 (2^31 - 1 itself: test_padded_int32_wide_id_truncated_away)"""
    import torch
    rows = _want_docs(case_name, map_name)[1]
    assert max(map(max, rows)) < 1 << 31
    _check_padded(_tok(case_name, map_name), list(_docs(case_name)), rows, torch.int32)


# ---------------------------------------------------------------------- int32 rows refuse ids >= 2^31
def _limit_error(excinfo, want_id):
    msg = str(excinfo.value)
    assert f"({_lib.BPE_E_LIMIT})" in msg and str(want_id) in msg, msg


@pytest.mark.parametrize("case_name,map_name", [("constructed", "top"), ("natural", "top"),
                                                ("constructed", f"edge:{V.T2}")])
def test_padded_int32_refuses_wide_ids(case_name, map_name):
    """An id an int32 cannot hold is an error, as in the uint16 output (bpe_ids_to_u16_device),
    and never a negative number; the message names the smallest such id among those kept."""
    import torch
    tok, docs = _tok(case_name, map_name), list(_docs(case_name))
    rows = _want_docs(case_name, map_name)[1]
    for T, truncation in ((None, "right"), (9, "right"), (8, "left")):   # (9: element stores, 8: 16-byte stores)
        kept = [r if T is None else r[:T] if truncation == "right" else r[-T:] for r in rows]
        wide = [i for r in kept for i in r if i >= 1 << 31]
        assert wide
        with pytest.raises(RuntimeError) as e:
            tok.encode_batch_padded(docs, T, pad_id=0, truncation=truncation, dtype=torch.int32)
        _limit_error(e, min(wide))
    got, _lengths = tok.encode_batch_padded(docs, 8, pad_id=0, dtype=torch.int64)   # the handle still works
    assert got.cpu().numpy().tolist() == [r[:8] + [0] * (8 - len(r[:8])) for r in rows]


def test_padded_int32_wide_id_truncated_away():
    """edge(2^31): p is 2^31, x is 2^31 + 1, q and the newline are below.  A row whose only wide
    id falls to the truncation is fine on either side; kept, it fails with the smallest one."""
    import torch
    tok = _tok("constructed", f"edge:{V.T2}")
    f = _map("constructed", f"edge:{V.T2}")
    q, p, x, nl = f[ord("q")], f[ord("p")], f[ord("x")], f[ord("\n")]
    assert (q, p, x) == (V.T2 - 1, V.T2, V.T2 + 1)
    last, first = "\nq\nq\nq\np", "\np\nq\nq\nq"          # 8 one-byte words each
    assert tok.encode_batch([last, first, "\nx\np"]) == [[nl, q] * 3 + [nl, p], [nl, p] + [nl, q] * 3, [nl, x, nl, p]]
    got, lengths = tok.encode_batch_padded([last, "\nq"], 7, pad_id=-1, truncation="right", dtype=torch.int32)
    assert got.cpu().numpy().tolist() == [[nl, q] * 3 + [nl], [nl, q] + [-1] * 5] and lengths.tolist() == [7, 2]
    got, lengths = tok.encode_batch_padded([first, "\nq"], 6, pad_id=-1, truncation="left", dtype=torch.int32)
    assert got.cpu().numpy().tolist() == [[nl, q] * 3, [nl, q] + [-1] * 4] and lengths.tolist() == [6, 2]
    assert int(got.max()) == (1 << 31) - 1              # the largest id an int32 holds is kept
    for docs, T, truncation in (([last], 8, "right"), ([first], 7, "left"), ([first], 2, "right"), ([last], 1, "left")):
        with pytest.raises(RuntimeError) as e:
            tok.encode_batch_padded(docs + ["\nq"], T, pad_id=-1, truncation=truncation, dtype=torch.int32)
        _limit_error(e, p)
    with pytest.raises(RuntimeError) as e:                 # two wide ids: the smaller is named
        tok.encode_batch_padded(["\nx\np", "\nx"], 4, pad_id=-1, dtype=torch.int32)
    _limit_error(e, p)
    with pytest.raises(RuntimeError) as e:
        tok.encode_batch_padded(["\nx\np", "\nx"], 3, pad_id=-1, dtype=torch.int32)
    _limit_error(e, x)
    with pytest.raises(RuntimeError, match=rf"\({_lib.BPE_E_ARG}\)"):   # pad_id: its own check, as before
        tok.encode_batch_padded(["\nq"], 4, pad_id=1 << 31, dtype=torch.int32)


@pytest.mark.parametrize("row_len", [8, 7])   # 16-byte stores / element stores
def test_pack_rows_int32_direct(row_len):
    import torch
    L = _lib.lib()
    big = (1 << 32) - 1
    rows = [[1, 2, 3], list(range(10, 10 + row_len)) + [1 << 31], [], [5, big], [(1 << 31) - 1] * (row_len + 2)]
    flat = np.array([i for r in rows for i in r], dtype=np.uint32)
    d_ids = torch.from_numpy(flat.view(np.int32).copy()).cuda()
    offsets = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    lengths = torch.zeros(len(rows), dtype=torch.int32, device="cuda")

    def pack(first, count, flags, elem):
        """rows first .. first + count - 1"""
        out = torch.empty((count, row_len), dtype=torch.int32 if elem == 4 else torch.int64, device="cuda")
        off = torch.from_numpy(offsets[first:first + count + 1].copy()).cuda()
        torch.cuda.synchronize()
        rc = L.bpe_ids_pack_rows_device(ctypes.c_void_p(d_ids.data_ptr()), ctypes.c_void_p(off.data_ptr()), count,
                                        row_len, -1, flags, elem, ctypes.c_void_p(out.data_ptr()),
                                        ctypes.c_void_p(lengths.data_ptr()), None)
        return rc, out.cpu().numpy(), (L.bpe_last_error() or b"").decode()

    rc, _out, msg = pack(0, 5, 0, 4)              # keep first: 2^32 - 1 of row 3 is kept, 2^31 of row 1 is not
    assert rc == _lib.BPE_E_LIMIT and str(big) in msg, msg
    rc, _out, msg = pack(0, 5, 1, 4)              # keep last: both are kept, the smaller is named
    assert rc == _lib.BPE_E_LIMIT and str(1 << 31) in msg and str(big) not in msg, msg
    rc, out, _msg = pack(0, 3, 0, 4)              # rows 0-2: the wide id of row 1 is truncated away
    assert rc == 0 and out.tolist() == [[1, 2, 3] + [-1] * (row_len - 3), list(range(10, 10 + row_len)), [-1] * row_len]
    rc, out, _msg = pack(4, 1, 2, 4)              # 2^31 - 1 fits
    assert rc == 0 and out.tolist() == [[(1 << 31) - 1] * row_len]
    rc, out, _msg = pack(0, 5, 1, 8)              # int64 rows hold every id
    assert rc == 0 and out[3].tolist() == [5, big] + [-1] * (row_len - 2)
    assert out[1].tolist() == list(range(11, 10 + row_len)) + [1 << 31]


# ---------------------------------------------------------------------- ranks, files, decode, create
def test_two_ranks_keep_the_ids(monkeypatch):
    """The per-rank copies of the tokenizer are rebuilt from the stored vocab and merges."""
    monkeypatch.setenv("BPE355_INPROC_RANKS", "1")
    for case_name in V.CASES:
        tok = _new_tok(case_name, "scatter")
        text = V.CASES[case_name]().text
        one = tok.encode(text)
        try:
            bpe_amd.set_num_gpus(2)
            two = tok.encode(text)
        finally:
            bpe_amd.set_num_gpus(None)
        _check(one, case_name, "scatter")
        assert two == one


@pytest.mark.parametrize("case_name", list(V.CASES))
def test_encode_file_uint16(case_name, tmp_path):
    """straddle(2^15): ids around 32 768, all within uint16"""
    from bpe_amd.encode import encode_file
    map_name = f"straddle:{V.T4}"
    want = _want(case_name, map_name)[1]
    assert (1 << 15) <= max(want) < (1 << 16) and min(want) < (1 << 15)
    src = tmp_path / "text.txt"
    src.write_bytes(V.CASES[case_name]().text.encode("utf-8"))
    got = encode_file(_tok(case_name, map_name), src)
    assert got.dtype == np.uint16 and got.tolist() == want


@pytest.mark.parametrize("case_name", list(V.CASES))
def test_decode_sparse_ids(case_name):
    """ids up to 7919 * n + 17 < 2^22.  (The constructed text without its missing special: the
    reference's vocab has no entry under that id, decode raises KeyError for it.)"""
    c = V.CASES[case_name]()
    f = _map(case_name, "sparse22")
    assert 1 << 21 < max(f.values()) < 1 << 22
    tok = _new_tok(case_name, "sparse22")
    text = c.text.replace(V.SP_MISSING, "")
    ids = tok.encode(text)
    assert ids == [f[i] for i in oracle.encode(c.vocab, c.merges, c.specials, text)]
    assert tok.decode(ids) == text
    docs = V.cut_documents(text, N_DOCS, 12)
    rows = tok.encode_batch(docs)
    assert tok.decode_batch(rows) == docs
    if case_name == "constructed":
        with pytest.raises(KeyError):
            tok.decode([c.n])


def test_decode_limit_with_top_ids():
    """encode takes ids up to 2^32 - 1; the decoder's table takes ids below 2^28 and says so."""
    tok = _tok("natural", "top")
    ids = tok.encode("the cat sat")
    assert ids and min(ids) >= (1 << 32) - 500
    with pytest.raises(RuntimeError, match=rf"\({_lib.BPE_E_LIMIT}\).*2\^28"):
        tok.decode(ids)
    with pytest.raises(RuntimeError, match=rf"\({_lib.BPE_E_LIMIT}\).*2\^28"):
        tok.decode_batch([ids])


@pytest.mark.parametrize("bad", [1 << 32, -1])
def test_create_refuses_ids_outside_u32(bad):
    vocab = {i: bytes([i]) for i in range(256)}
    vocab[bad] = b"ab"
    tok = bpe_amd.Tokenizer(vocab, [(b"a", b"b")], [])
    with pytest.raises(RuntimeError, match=rf"\({_lib.BPE_E_ARG}\).*2\^32"):
        tok.encode("ab")
