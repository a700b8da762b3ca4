"""GPU: the id emit of the encoder (k_enc_emit, k_enc_cut_offsets) and the word loads in front of
it (load_word, enc_table_add, k_encode_words; csrc/encode.hip) against the C oracle, on the inputs
of tests/emit_cases.py; tests/test_emit_cases.py shows on the CPU which parts, paths and
boundaries they reach.  Every comparison is exact equality of id arrays; a failure names the first
differing index and the chunk, part and path the plan assigns to it.

  uint32 ids          Tokenizer.encode and encode_batch_np of every case; encode_files with uint32
  uint16 ids          encode_file(fmt="bin") and encode_files with uint16 of every case
  finalize modes      BPE355_ENC_FINALIZE 0, unset and 2, with and without the scan's LDS cache
                      (BPE355_NOCACHE: every word a pending entry), uint32 and uint16
  uint16 refusals     one id of 70 000 in a head element, an even and an odd slot of a packed pair,
                      a tail element, a path-(b) part, the first and a later round of a path-(c)
                      part: each the documented limit error and no output file; the same text
                      without the wide byte encodes
  cut offsets         encode_batch_np with document starts at records 0, 1, 2047, 2048, 2049, 4095,
                      4096 and the last of every part (so r0 - 1, r0, r0 + 1 of every seam), at the
                      first record after an empty chunk, and a run of empty documents
  workgroup reuse     mixed_reuse sized from the device's CU count so that the emit's grid-stride
                      loop is re-entered, uint32 (encode_batch_np) and uint16 (encode_file),
                      against the tiling of one block's oracle ids
  word loads          Tokenizer.encode, bpe_tok_encode_device on pointers 1, 3, 8 and 15 bytes
                      past a 16-byte boundary, BPE355_NOCACHE=1 and BPE355_ENC_PEND_CAP=0; the
                      1025 texts of word_load_tails() (a last word of 1..40 bytes with 0..24 bytes
                      after it), each under the same three knob sets

Measured on an MI355X (256 CUs: mixed_reuse is 854 blocks, 42 MB, 5126 parts against a grid of at
most 4096 workgroups): the 79 tests take 6.6 s together; the slowest step is the set-up of the
first test, which loads the library (1.5 s); of the tests test_word_load_tails takes 0.29 to 0.36 s
per knob set (1025 encodes each), test_encode_uint32[path_a_edges] 0.29 s, the two reuse runs
0.07 s each after 0.13 s of set-up (the text, its plan and the tiled expectation), every other
0.16 s or less, oracle runs included.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

import bpe_amd
import emit_cases as E
from bpe_amd import _lib
from oracle import oracle

pytestmark = pytest.mark.gpu

ONE_PIECE = 1 << 40          # chars_per_piece: the whole file is one piece
SHIFTS = (1, 3, 8, 15)
CUT_CASES = ("records_edge", "path_b", "empty_chunks")
FINALIZE = [{"BPE355_ENC_FINALIZE": "0"}, {}, {"BPE355_ENC_FINALIZE": "2"},
            {"BPE355_ENC_FINALIZE": "0", "BPE355_NOCACHE": "1"}, {"BPE355_NOCACHE": "1"},
            {"BPE355_ENC_FINALIZE": "2", "BPE355_NOCACHE": "1"}]


def _knob_id(k):
    return ",".join(f"{a}={b}" for a, b in k.items()) or "default"


@pytest.fixture(scope="module", autouse=True)
def _device():
    _lib.require_device()


def _encode(vocab, text):
    return np.array(oracle.encode(vocab, E.merges(), E.SPECIALS, text), dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def _want(name):
    """the oracle's ids of a case, computed once and shared (read-only)"""
    ids = _encode(E.vocab(), E.CASES[name]())
    ids.setflags(write=False)
    return ids


@functools.lru_cache(maxsize=None)
def _plan(name):
    return E.plan_of(E.CASES[name]())


def _new_tok(vocab=None):
    return bpe_amd.Tokenizer(E.vocab() if vocab is None else vocab, E.merges(), list(E.SPECIALS))


@functools.lru_cache(maxsize=None)
def _tok():
    return _new_tok()


@functools.lru_cache(maxsize=None)
def _wide_tok():
    return _new_tok(E.wide_vocab())


def _same(got, want, plan=None):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape == want.shape and np.array_equal(got, want):
        return
    n = min(len(got), len(want))
    d = np.flatnonzero(got[:n] != want[:n])
    k = int(d[0]) if d.size else n
    where = f"; {plan.locate(k)}" if plan is not None else ""
    pytest.fail(f"{len(got)} ids against {len(want)}, first difference at {k}: {got[k:k + 6].tolist()} against "
                f"{want[k:k + 6].tolist()}{where}")


def _write(tmp_path, name, text):
    src = tmp_path / name
    src.write_bytes(text.encode("utf-8"))
    return src


# ---------------------------------------------------------------------- uint32 and uint16, every case
@pytest.mark.parametrize("name", list(E.CASES))
def test_encode_uint32(name):
    text = E.CASES[name]()
    _same(np.array(_tok().encode(text), dtype=np.uint32), _want(name), _plan(name))
    ids, offsets = _tok().encode_batch_np([text])
    assert ids.dtype == np.uint32 and offsets.tolist() == [0, len(_want(name))]
    _same(ids, _want(name), _plan(name))


@pytest.mark.parametrize("name", list(E.CASES))
def test_encode_file_uint16(name, tmp_path):
    from bpe_amd.encode import encode_file
    src, out = _write(tmp_path, "text.txt", E.CASES[name]()), tmp_path / "ids.bin"
    got = encode_file(_tok(), src, out, fmt="bin", chars_per_piece=ONE_PIECE)
    assert got.dtype == np.uint16
    _same(got, _want(name), _plan(name))
    _same(np.fromfile(out, np.uint16), _want(name), _plan(name))


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["uint16", "uint32"])
@pytest.mark.parametrize("name", list(E.CASES))
def test_encode_files(name, dtype, tmp_path):
    src, out = _write(tmp_path, "text.txt", E.CASES[name]()), tmp_path / "ids.bin"
    res = bpe_amd.encode_files(_tok(), [src], out, dtype=dtype, chars_per_piece=ONE_PIECE)
    assert res["n_ids"] == len(_want(name)) and res["n_pieces"] == 1 and res["n_windows"] == 1
    _same(np.fromfile(out, dtype), _want(name), _plan(name))


@pytest.mark.parametrize("knobs", FINALIZE, ids=_knob_id)
@pytest.mark.parametrize("name", list(E.CASES))
def test_finalize_modes(name, knobs, monkeypatch, tmp_path):
    """rec_info's three shapes and the count pass's write-back"""
    from bpe_amd.encode import encode_file
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    tok, text = _new_tok(), E.CASES[name]()
    _same(np.array(tok.encode(text), dtype=np.uint32), _want(name), _plan(name))
    got = encode_file(tok, _write(tmp_path, "text.txt", text), chars_per_piece=ONE_PIECE)
    assert got.dtype == np.uint16
    _same(got, _want(name), _plan(name))


# ---------------------------------------------------------------------- uint16 refusals
def _refused(excinfo):
    msg = str(excinfo.value)
    assert f"({_lib.BPE_E_LIMIT})" in msg and "uint16" in msg, msg


@pytest.mark.parametrize("region", E.REFUSAL_REGIONS)
def test_uint16_refusal(region, tmp_path):
    """The wide id occurs once; each of the places where k_enc_emit<uint16_t> narrows an id must
    report it (status bit 128) on its own."""
    from bpe_amd.encode import encode_file
    text = E.refusal_text(region)
    want = _encode(E.wide_vocab(), text)
    assert int((want > 0xFFFF).sum()) == 1
    plan = E.plan_of(text)
    k = int(np.flatnonzero(want > 0xFFFF)[0])
    assert E._refusal_class(plan.region(k, 2)) == region
    tok = _wide_tok()
    src, out = _write(tmp_path, "wide.txt", text), tmp_path / "wide.bin"
    with pytest.raises(RuntimeError) as e:
        encode_file(tok, src, out, fmt="bin", chars_per_piece=ONE_PIECE)
    _refused(e)
    assert not out.exists(), plan.locate(k)
    with pytest.raises(RuntimeError) as e:
        bpe_amd.encode_files(tok, [src], out, dtype=np.uint16, chars_per_piece=ONE_PIECE)
    _refused(e)
    assert not out.exists() and sorted(x.name for x in tmp_path.iterdir()) == ["wide.txt"]
    _same(np.array(tok.encode(text), dtype=np.uint32), want, plan)   # the handle still works; uint32 holds the id


def test_uint16_refusal_control(tmp_path):
    """the same text without the wide byte, the same tokenizer: uint16 ids, equal to the oracle's"""
    from bpe_amd.encode import encode_file
    text = E.refusal_base()
    want, plan = _encode(E.wide_vocab(), text), E.plan_of(text)
    src, out = _write(tmp_path, "base.txt", text), tmp_path / "base.bin"
    got = encode_file(_wide_tok(), src, out, fmt="bin", chars_per_piece=ONE_PIECE)
    _same(got, want, plan)
    _same(np.fromfile(out, np.uint16), want, plan)
    res = bpe_amd.encode_files(_wide_tok(), [src], out, dtype=np.uint16, chars_per_piece=ONE_PIECE)
    assert res["n_ids"] == len(want)
    _same(np.fromfile(out, np.uint16), want, plan)


# ---------------------------------------------------------------------- cut offsets
ROUND_EDGES = (0, 1, E.K_CUT_ROUND - 1, E.K_CUT_ROUND, E.K_CUT_ROUND + 1, 2 * E.K_CUT_ROUND - 1, 2 * E.K_CUT_ROUND)


@functools.lru_cache(maxsize=None)
def _cut_docs(name):
    """(documents, expected rows): document starts at the records ROUND_EDGES and the last one of
    every part -- with records 0 and 1 of part 1 and the last of part 0 that is r0 - 1, r0, r0 + 1
    of every seam -- and at the first record after an empty chunk; three empty documents at the
    deepest round edge"""
    text, p = E.CASES[name](), _plan(name)
    data = text.encode()
    recs = set()
    for j in range(len(p.m)):
        m, lo = int(p.m[j]), int(p.lo[j])
        recs |= {lo + k for k in ROUND_EDGES + (m - 1,) if 0 <= k < m}
    after_empty = [int(p.lo[2 * c]) for c in range(1, len(p.mc)) if p.mc[c - 1] == 0 and p.mc[c] > 0]
    recs |= set(after_empty)
    if name == "empty_chunks":
        assert after_empty, "a document start at the first record after an empty chunk"
    cuts = sorted({int(p.starts[r]) for r in recs} - {0})
    starts, _lens, nids = E.records(data, cuts)
    assert np.array_equal(starts, p.starts) and np.array_equal(nids, p.nids)   # the cuts leave the plan as it is
    deep = max(recs, key=lambda r: (r - int(p.lo[np.searchsorted(p.lo, r, "right") - 1]), r))
    docs = []
    for a, b in zip([0] + cuts, cuts + [len(data)]):
        if a == int(p.starts[deep]):
            docs += ["", "", ""]
        docs.append(data[a:b].decode())
    memo: dict = {}
    rows = []
    for d in docs:
        if d not in memo:
            memo[d] = _encode(E.vocab(), d)
        rows.append(memo[d])
    return docs, rows


@pytest.mark.parametrize("knobs", [{}, {"BPE355_ENC_FINALIZE": "0"}, {"BPE355_ENC_FINALIZE": "2"}], ids=_knob_id)
@pytest.mark.parametrize("name", CUT_CASES)
def test_cut_offsets(name, knobs, monkeypatch):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    docs, rows = _cut_docs(name)
    assert "" in docs and len(docs) > 20
    if name == "records_edge":   # cuts at both sides of every round edge of a four-round part
        p = _plan(name)
        assert p.m[0] == 4 * E.K_CUT_ROUND and p.m[2] == 2 * E.K_CUT_ROUND
    ids, offsets = _new_tok().encode_batch_np(docs)
    want_off = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    bad = np.flatnonzero(offsets != want_off)
    assert bad.size == 0, (f"{bad.size} offsets differ, the first at document {int(bad[0])}: {int(offsets[bad[0]])} against "
                           f"{int(want_off[bad[0]])}; {_plan(name).locate(int(want_off[bad[0]]))}")
    _same(ids, np.concatenate(rows), _plan(name))
    for i, r in enumerate(rows):
        assert np.array_equal(ids[offsets[i]:offsets[i + 1]], r), i
    _same(ids, _want(name), _plan(name))   # cuts at record starts: the ids of the whole text


# ---------------------------------------------------------------------- word loads
@pytest.mark.parametrize("knobs", [{}, {"BPE355_NOCACHE": "1"}, {"BPE355_ENC_PEND_CAP": "0"}], ids=_knob_id)
def test_word_loads(knobs, monkeypatch):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    tok = _new_tok()
    _same(np.array(tok.encode(E.word_loads()), dtype=np.uint32), _want("word_loads"), _plan("word_loads"))


@pytest.mark.parametrize("shift", SHIFTS)
def test_word_loads_device_unaligned(shift):
    import torch
    data = E.word_loads().encode("utf-8")
    n = len(data)
    buf = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[shift:shift + n] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    out = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    n_out = ctypes.c_size_t(0)
    _lib.check(_lib.lib().bpe_tok_encode_device(_tok()._device(), ctypes.c_void_p(buf.data_ptr() + shift), n,
                                                ctypes.c_void_p(out.data_ptr()), ctypes.byref(n_out), None), "encode")
    torch.cuda.synchronize()
    _same(out[:n_out.value].cpu().numpy().view(np.uint32), _want("word_loads"), _plan("word_loads"))


@functools.lru_cache(maxsize=None)
def _tails_want():
    return tuple(_encode(E.vocab(), t) for t in E.word_load_tails())


@pytest.mark.parametrize("knobs", [{}, {"BPE355_NOCACHE": "1"}, {"BPE355_ENC_PEND_CAP": "0"}], ids=_knob_id)
def test_word_load_tails(knobs, monkeypatch):
    """the last word of a text with 0..24 bytes after it: load_word's byte path and its complement"""
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    tok = _new_tok()
    for text, want in zip(E.word_load_tails(), _tails_want()):
        got = np.array(tok.encode(text), dtype=np.uint32)
        if not np.array_equal(got, want):
            s, ln, after = E.last_word(text.encode())
            pytest.fail(f"last word of {ln} bytes at {s} with {after} bytes after it: {got.tolist()} against {want.tolist()}")


# ---------------------------------------------------------------------- workgroup reuse
# (last in the module: the fixture's text, expectation and plan are freed when these two are done)
@pytest.fixture(scope="module")
def reuse():
    """(text, expected ids, plan) at the size at which the emit's workgroups take several parts"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    reps = E.reuse_reps(cus)
    plan = E.reuse_plan(reps)
    n_parts = len(plan.m)
    print(f"mixed_reuse: {cus} CUs, {reps} blocks, {reps * E.BLOCK_BYTES} bytes, {n_parts} parts")
    assert n_parts >= 1.25 * (E.MAX_WG_PER_CU * cus * 2)
    later = plan.path()[E.MAX_WG_PER_CU * cus * 2:]
    assert set(later.tolist()) == {"a", "b", "c"}
    plan.drop_records()   # locate() needs the per-part arrays alone
    want = np.tile(_encode(E.vocab(), E.reuse_block()), reps)
    return E.mixed_reuse(reps), want, plan


def test_reuse_uint32(reuse):
    text, want, plan = reuse
    ids, offsets = _tok().encode_batch_np([text])
    assert offsets.tolist() == [0, len(want)]
    _same(ids, want, plan)


def test_reuse_uint16(reuse, tmp_path):
    from bpe_amd.encode import encode_file
    text, want, plan = reuse
    src, out = _write(tmp_path, "reuse.txt", text), tmp_path / "reuse.bin"
    got = encode_file(_tok(), src, out, fmt="bin", chars_per_piece=ONE_PIECE)
    assert got.dtype == np.uint16
    _same(got, want, plan)
    _same(np.memmap(out, np.uint16, "r"), want, plan)
