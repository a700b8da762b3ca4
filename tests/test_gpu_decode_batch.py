"""Tokenizer.decode_batch / decode_batch_bytes / decode_batch_np / decode_batch_padded /
decode_tokens (bpe_dec_decode_batch, bpe_dec_decode_batch_device, bpe_dec_decode_rows_device): many
rows of ids decoded in one launch sequence, each row exactly as a separate decode().

The oracle is the reference's own rule per row (tokenizer.py:155-157),
b"".join(vocab[i] for i in row).decode("utf-8", errors="replace"), on the GPT-2 fixture vocab.  The
shapes sit on and next to the gather's tile (2048 ids, 16 KiB of LDS per workgroup), on every
alignment of the output's first byte, and in tiles whose bytes do not fit the LDS buffer.
"""
from __future__ import annotations

import ctypes
import functools
import random

import numpy as np
import pytest

import gpt2_files

pytestmark = pytest.mark.gpu

bpe_amd = pytest.importorskip("bpe_amd")
from bpe_amd import _lib  # noqa: E402

EOT = ["<|endoftext|>"]
P = ctypes.c_void_p
TILE_IDS, TILE_BYTES = 2048, 16384   # kDecTileIds, kDecTileBytes of csrc/decode.hip


@functools.lru_cache(maxsize=None)
def _gpt2():
    vocab, merges = gpt2_files.load_gpt2(EOT)
    return vocab, merges, bpe_amd.Tokenizer(dict(vocab), list(merges), EOT)


def _ref_bytes(vocab, row):
    return b"".join([vocab[i] for i in row])


def _ref(vocab, row):
    return _ref_bytes(vocab, row).decode("utf-8", errors="replace")


def _random_ids(rng, vocab, n):
    """ids of the whole vocab, a quarter of them single-byte ids (they split UTF-8 sequences)"""
    all_ids = sorted(vocab)
    single = [i for i in all_ids if len(vocab[i]) == 1]
    return [rng.choice(single) if rng.random() < 0.25 else rng.choice(all_ids) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def _seam_rows():
    """(rows, index k of the row that ends inside a 3-byte character); computed once, read-only"""
    vocab, _, _ = _gpt2()
    rng = random.Random(20250101)
    lens = [0, 0, 1, 1000] + [rng.choice((0, 1, 2, 7, 63, 64, 65, 255, 256, 257, 1000)) for _ in range(40)]
    lens += [64, 0, 0, 257, 2, 0]   # empty rows first, last and twice in a row
    assert {0, 1, 2, 7, 63, 64, 65, 255, 256, 257, 1000} <= set(lens)
    rows = [_random_ids(rng, vocab, n) for n in lens]
    inv = {b: i for i, b in vocab.items()}
    b0, b1, b2 = (inv[bytes([b])] for b in "世".encode("utf-8"))
    k = 10
    rows[k] = rows[k] + [inv[b"a"], b0, b1]     # two bytes of the character end row k ...
    rows[k + 1] = [b2, inv[b"b"]] + rows[k + 1]  # ... the third begins row k + 1
    return tuple(tuple(r) for r in rows), k


def test_rows_and_seams():
    vocab, _, tok = _gpt2()
    rows, k = _seam_rows()
    assert rows[0] == () and rows[1] == () and rows[-1] == ()
    want_b = [_ref_bytes(vocab, r) for r in rows]
    want = [b.decode("utf-8", errors="replace") for b in want_b]
    # the split character is replacement characters in both rows, and would not be in the join
    assert want[k].endswith("a�") and want[k + 1].startswith("�b")
    assert "世" in (want_b[k] + want_b[k + 1]).decode("utf-8", errors="replace")
    lists = [list(r) for r in rows]
    assert tok.decode_batch(lists) == want
    assert tok.decode_batch(rows) == want            # tuples as rows
    assert tok.decode_batch_bytes(lists) == want_b
    ids = np.array([i for r in rows for i in r], dtype=np.uint32)
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    data, byte_off = tok.decode_batch_np(ids, offsets)
    assert data.dtype == np.uint8 and byte_off.dtype == np.int64 and byte_off.shape == (len(rows) + 1,)
    assert byte_off[0] == 0 and byte_off[-1] == data.size == sum(map(len, want_b))
    for i, b in enumerate(want_b):
        assert data[byte_off[i]:byte_off[i + 1]].tobytes() == b, i
    assert want[3] == tok.decode(lists[3])   # the same string a separate decode() gives


def test_zero_rows_and_all_empty_rows():
    _, _, tok = _gpt2()
    assert tok.decode_batch([]) == [] and tok.decode_batch_bytes([]) == [] and tok.decode_tokens([]) == []
    assert tok.decode_batch([[], [], []]) == ["", "", ""]
    assert tok.decode_batch_bytes([[], []]) == [b"", b""]
    data, byte_off = tok.decode_batch_np(np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.int64))
    assert data.shape == (0,) and byte_off.tolist() == [0]
    data, byte_off, tok_off = tok.decode_batch_np(np.zeros(0, dtype=np.uint32), np.zeros(4, dtype=np.int64), True)
    assert data.shape == (0,) and byte_off.tolist() == [0, 0, 0, 0] and tok_off.tolist() == [0]


# ---------------------------------------------------------------------- tile and alignment edges
EDGE_TOTALS = sorted(set(range(0, 70)) | {k + d for k in (256, 1024, 2048, 4096, 8192, 16384) for d in (-1, 0, 1)})
GUARD = 0xA5


@functools.lru_cache(maxsize=None)
def _edge_ids():
    vocab, _, _ = _gpt2()
    ids = _random_ids(random.Random(77), vocab, max(EDGE_TOTALS))
    lens = np.array([len(vocab[i]) for i in ids], dtype=np.int64)
    return tuple(ids), b"".join(vocab[i] for i in ids), np.concatenate([[0], np.cumsum(lens)])


def _batch_device(tok, d_ids, n, d_off, n_rows, d_out, cap, d_byte_off, d_tok_off, stream=None):
    n_out = ctypes.c_size_t(0)
    rc = _lib.lib().bpe_dec_decode_batch_device(tok._decoder(), P(d_ids.data_ptr()), n, P(d_off.data_ptr()), n_rows,
                                                d_out, cap, ctypes.byref(n_out), P(d_byte_off.data_ptr()),
                                                P(d_tok_off.data_ptr()) if d_tok_off is not None else None, stream)
    return rc, n_out.value


def test_tile_and_alignment_edges():
    import torch
    _, _, tok = _gpt2()
    ids, all_bytes, cum = _edge_ids()
    n_max = len(ids)
    d_ids = torch.tensor(ids, dtype=torch.int64, device="cuda").to(torch.int32)   # uint32 bit patterns
    d_all = torch.frombuffer(bytearray(all_bytes), dtype=torch.uint8).cuda()
    cap_max = len(all_bytes)
    buf = torch.empty(64 + 16 + cap_max + 64, dtype=torch.uint8, device="cuda")
    want = torch.empty_like(buf)
    d_byte_off = torch.empty(4, dtype=torch.int64, device="cuda")
    d_tok_off = torch.empty(n_max + 1, dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    base = buf.data_ptr()
    assert base % 16 == 0
    for n in EDGE_TOTALS:
        total = int(cum[n])
        offs = [0, n // 3, n // 3, n]     # three rows, the middle one empty
        d_off = torch.tensor(offs, dtype=torch.int64, device="cuda")
        for shift in range(16):
            lo = 64 + shift
            buf.fill_(GUARD)
            want.fill_(GUARD)
            want[lo:lo + total] = d_all[:total]
            torch.cuda.synchronize()
            stream = P(side.cuda_stream) if (n, shift) == (4097, 5) else None   # once: not the decoder's own stream
            rc, got = _batch_device(tok, d_ids, n, d_off, 3, P(base + lo), total, d_byte_off,
                                    d_tok_off if shift == 3 else None, stream)
            assert rc == 0 and got == total, (n, shift, rc)
            assert torch.equal(buf, want), (n, shift)   # the bytes, and the guard bytes before and after
            if shift in (0, 3):
                assert d_byte_off.tolist() == [int(cum[o]) for o in offs], (n, shift)
            if shift == 3:
                assert d_tok_off[:n + 1].tolist() == cum[:n + 1].tolist(), n


# ---------------------------------------------------------------------- long tokens
@functools.lru_cache(maxsize=None)
def _long_tok():
    vocab = {i: bytes([i]) for i in range(256)}
    vocab[256] = bytes(range(65, 82))                                   # 17 bytes
    vocab[257] = bytes((7 * i + 1) % 251 for i in range(4096))
    vocab[258] = bytes((11 * i + 3) % 253 for i in range(70_000))
    return vocab, bpe_amd.Tokenizer(dict(vocab), [], [])


def test_long_tokens_overflow_the_lds_buffer():
    vocab, tok = _long_tok()
    rng = random.Random(5)

    def singles(n):
        return [rng.randrange(256) for _ in range(n)]

    tiles = [
        singles(TILE_IDS),                                                # fits: one byte per id
        singles(TILE_IDS),
        singles(700) + [258] + singles(300) + [256, 257] + singles(TILE_IDS - 1003),   # one 70 000-byte entry
        [256] * TILE_IDS,                                                 # 34 816 bytes of short tokens: straight to memory
        singles(1000) + [257, 257, 257] + singles(TILE_IDS - 1003),       # 12 288 + 2045 bytes: still fits
        [257] * 5 + singles(TILE_IDS - 5),                                # 20 480 + 2043 bytes: does not
        [258, 256, 258] + singles(40),                                    # the last, partial tile
    ]
    sizes = [sum(len(vocab[i]) for i in t) for t in tiles]
    assert [s + 15 <= TILE_BYTES for s in sizes] == [True, True, False, False, True, False, False]
    flat = [i for t in tiles for i in t]
    cuts = sorted(rng.sample(range(1, len(flat)), 30))
    rows = [flat[a:b] for a, b in zip([0] + cuts, cuts + [len(flat)])]
    want = [_ref_bytes(vocab, r) for r in rows]
    assert tok.decode_batch_bytes(rows) == want
    assert tok.decode_batch(rows) == [b.decode("utf-8", errors="replace") for b in want]
    # a buffer that does not start a tile on a 16-byte boundary of the output
    assert tok.decode_batch_bytes([[5]] + rows) == [b"\x05"] + want


# ---------------------------------------------------------------------- token offsets
def test_token_offsets():
    vocab, _, tok = _gpt2()
    rows, _ = _seam_rows()
    ids = np.array([i for r in rows for i in r], dtype=np.uint32)
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    data, byte_off, t = tok.decode_batch_np(ids, offsets, return_token_offsets=True)
    assert t.dtype == np.int64 and t.shape == (ids.size + 1,)
    raw = data.tobytes()
    tl = t.tolist()
    for j, i in enumerate(ids.tolist()):
        assert raw[tl[j]:tl[j + 1]] == vocab[i], j
    assert byte_off.tolist() == [tl[o] for o in offsets.tolist()]
    assert tl[-1] == len(raw)


# ---------------------------------------------------------------------- errors
@functools.lru_cache(maxsize=None)
def _gap_tok():
    vocab = {i: bytes([i]) for i in range(256) if i != 100}
    vocab[300] = b"xyz"   # ids 256..299 are a gap, the table ends at 300
    return vocab, bpe_amd.Tokenizer(dict(vocab), [], [])


def _raised(fn):
    with pytest.raises(Exception) as e:
        fn()
    return type(e.value), e.value.args


@pytest.mark.parametrize("bad", [100, 270, 301, 70_000, 0xFFFFFFFF])
def test_missing_id_raises_keyerror_with_the_id(bad):
    _, tok = _gap_tok()
    for call in (tok.decode_batch, tok.decode_batch_bytes):
        with pytest.raises(KeyError) as e:
            call([[1, 2], [], [3, bad, 4]])
        assert e.value.args == (bad,)
    with pytest.raises(KeyError) as e:
        tok.decode_tokens([1, bad])
    assert e.value.args == (bad,)
    with pytest.raises(KeyError) as e:
        tok.decode_batch_np(np.array([1, bad], dtype=np.uint32), np.array([0, 1, 2]))
    assert e.value.args == (bad,)
    assert tok.decode_batch([[65, 300]]) == ["Axyz"]   # still usable


def test_first_bad_id_in_flat_order_is_reported():
    _, tok = _gap_tok()
    rows = [[1] * 3000, [2, 270, 3], [4] * 3000, [301]]
    with pytest.raises(KeyError) as e:
        tok.decode_batch(rows)
    assert e.value.args == (270,)
    with pytest.raises(KeyError) as e:
        tok.decode_batch(rows[::-1])
    assert e.value.args == (301,)


@pytest.mark.parametrize("bad", [-1, 2 ** 32, "x", 2 ** 70, 1.5, None])
def test_ids_decode_refuses_raise_the_same(bad):
    _, tok = _gap_tok()
    want = _raised(lambda: tok.decode([7, bad]))
    assert _raised(lambda: tok.decode_batch([[1, 2], [7, bad], [-5]])) == want
    assert _raised(lambda: tok.decode_batch_bytes([[7, bad]])) == want
    assert _raised(lambda: tok.decode_tokens([7, bad])) == want


def test_argument_errors_through_ctypes():
    import torch
    _, _, tok = _gpt2()
    L = _lib.lib()
    ids = np.array([15496, 11, 995, 0], dtype=np.uint32)
    byte_off = np.zeros(8, dtype=np.uint64)
    d_ids = torch.tensor(ids.astype(np.int64), device="cuda").to(torch.int32)
    d_byte_off = torch.empty(8, dtype=torch.int64, device="cuda")
    d_out = torch.empty(64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for offs in ([0, 3, 2, 4], [1, 2, 4], [0, 2, 3], [0, 2, 5]):   # decreasing, first not 0, last not n (twice)
        o = np.array(offs, dtype=np.uint64)
        p, nb = P(), ctypes.c_size_t(0)
        rc = L.bpe_dec_decode_batch(tok._decoder(), ids.ctypes.data, 4, o.ctypes.data, len(offs) - 1, ctypes.byref(p),
                                    ctypes.byref(nb), byte_off.ctypes.data, None)
        assert rc == _lib.BPE_E_ARG and not p.value, offs
        d_off = torch.tensor(offs, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        rc, _ = _batch_device(tok, d_ids, 4, d_off, len(offs) - 1, P(d_out.data_ptr()), 64, d_byte_off, None)
        assert rc == _lib.BPE_E_ARG, offs
    vocab = tok.vocab
    need = sum(len(vocab[int(i)]) for i in ids)
    d_off = torch.tensor([0, 1, 4], dtype=torch.int64, device="cuda")
    d_out.fill_(GUARD)
    torch.cuda.synchronize()
    rc, got = _batch_device(tok, d_ids, 4, d_off, 2, P(d_out.data_ptr()), need - 1, d_byte_off, None)
    assert rc == _lib.BPE_E_ARG and got == need
    assert bool((d_out == GUARD).all())          # nothing was written
    rc, got = _batch_device(tok, d_ids, 4, d_off, 2, P(d_out.data_ptr()), need, d_byte_off, None)
    assert rc == 0 and got == need
    assert bytes(d_out[:need].tolist()) == _ref_bytes(vocab, ids.tolist())
    # NULL required pointers
    assert L.bpe_dec_decode_batch(tok._decoder(), None, 0, None, 0, None, None, None, None) == _lib.BPE_E_ARG
    assert L.bpe_dec_decode_batch_device(tok._decoder(), None, 0, None, 0, None, 0, None, None, None, None) == _lib.BPE_E_ARG
    assert L.bpe_dec_decode_rows_device(tok._decoder(), None, 4, 0, 0, None, -1, 0, None, None, None, None) == _lib.BPE_E_ARG
    with pytest.raises(ValueError):
        tok.decode_batch_np(ids, np.array([0, 3, 2, 4]))


# ---------------------------------------------------------------------- padded rows
def _kept(row, length, T, stop_id, include_stop, side):
    """the kept span of one padded row, restated: the first `length` entries (left-padded: the
    last), all T without a length; cut before the first stop_id, or behind it"""
    length = T if length is None else length
    span = row[T - length:] if side == "left" else row[:length]
    if stop_id is not None and stop_id in span:
        span = span[:span.index(stop_id) + (1 if include_stop else 0)]
    return span


PAD = -100
T_PAD = 70   # more than one 64-entry round of the stop search


def _padded_case(side, with_lengths, stop_at):
    """-> (matrix as lists, lengths or None).  Ids are 1..255; 0 is the stop id, put at index
    stop_at[i] of row i's span (None: not in the row).  What lies outside the kept span is PAD."""
    rng = random.Random(1000 + 2 * (side == "left") + with_lengths)
    lengths = [T_PAD, 0, 1, 69, 66, 70, 33, 2, 64, 65]
    B = len(lengths)
    rows = []
    for i in range(B):
        L = lengths[i] if with_lengths else T_PAD
        span = [rng.randrange(1, 256) for _ in range(L)]
        s = stop_at.get(i)
        if s is not None and s < L:
            span[s] = 0
            if not with_lengths:          # without lengths, what follows the stop is outside the span
                span[s + 1:] = [PAD] * (L - s - 1)
        fill = [PAD] * (T_PAD - L)
        rows.append(fill + span if side == "left" else span + fill)
    return rows, (lengths if with_lengths else None)


@pytest.mark.parametrize("dtype", ["int32", "int64"])
@pytest.mark.parametrize("side", ["right", "left"])
@pytest.mark.parametrize("with_lengths", [True, False], ids=["lengths", "no-lengths"])
def test_padded_rows(dtype, side, with_lengths):
    import torch
    tok = bpe_amd.Tokenizer({i: bytes([i]) for i in range(256)}, [], [])
    tdt = getattr(torch, dtype)
    # no stop id in any row / at position 0, mid-row, past the first 64 entries, and absent elsewhere
    for stop_at in ({}, {0: 0, 3: 30, 4: 65, 5: 69, 6: 32, 9: 64}):
        rows, lengths = _padded_case(side, with_lengths, stop_at)
        x = torch.tensor(rows, dtype=tdt, device="cuda")
        lt = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device="cuda")
        for stop_id, include_stop in ((None, False), (0, False), (0, True), (999, False)):
            if stop_id != 0 and stop_at and not with_lengths:
                continue   # the PADs behind the stop id would be kept
            want = [_ref(tok.vocab, _kept(r, None if lengths is None else lengths[i], T_PAD, stop_id, include_stop,
                                          side)) for i, r in enumerate(rows)]
            got = tok.decode_batch_padded(x, lt, stop_id=stop_id, include_stop=include_stop, padding_side=side)
            assert got == want, (stop_at, stop_id, include_stop)
        if lengths is not None:
            assert tok.decode_batch_padded(x, lengths, padding_side=side) == tok.decode_batch_padded(
                x, lt, padding_side=side)   # lengths as a list


def test_padded_rows_errors_and_shapes():
    import torch
    tok = bpe_amd.Tokenizer({i: bytes([i]) for i in range(256)}, [], [])
    x = torch.tensor([[65, 66, PAD, PAD], [67, PAD, PAD, PAD], [68, 69, 70, 71]], dtype=torch.int64, device="cuda")
    lengths = torch.tensor([2, 1, 4], dtype=torch.int32, device="cuda")
    assert tok.decode_batch_padded(x, lengths) == ["AB", "C", "DEFG"]            # -100 outside the span: legal
    assert tok.decode_batch_padded(x.to(torch.int32), lengths) == ["AB", "C", "DEFG"]
    for dt in (torch.int32, torch.int64):
        with pytest.raises(KeyError) as e:
            tok.decode_batch_padded(x.to(dt), torch.tensor([2, 2, 4], dtype=torch.int32))   # inside it
        assert e.value.args == (PAD,)
    y = x.clone()
    y[2, 1] = 2 ** 32 + 5
    y[2, 3] = -7
    with pytest.raises(KeyError) as e:
        tok.decode_batch_padded(y, lengths)
    assert e.value.args == (2 ** 32 + 5,)
    y[0, 1] = 256   # no vocab entry, and earlier in row-major order
    with pytest.raises(KeyError) as e:
        tok.decode_batch_padded(y, lengths)
    assert e.value.args == (256,)
    for bad in (-1, 5):
        with pytest.raises(ValueError):
            tok.decode_batch_padded(x, torch.tensor([2, bad, 4], dtype=torch.int32))
    with pytest.raises(ValueError):
        tok.decode_batch_padded(x, lengths, padding_side="middle")
    with pytest.raises(ValueError):
        tok.decode_batch_padded(x.to(torch.float32), lengths)
    with pytest.raises(ValueError):
        tok.decode_batch_padded(x[0], lengths)
    assert tok.decode_batch_padded(torch.empty((3, 0), dtype=torch.int64, device="cuda")) == ["", "", ""]   # T == 0
    assert tok.decode_batch_padded(torch.empty((0, 5), dtype=torch.int32, device="cuda")) == []             # B == 0
    xt = torch.tensor([[65, 67, 68], [66, PAD, 69], [PAD, PAD, 70], [PAD, PAD, 71]], dtype=torch.int64, device="cuda").t()
    assert not xt.is_contiguous()
    assert tok.decode_batch_padded(xt, lengths) == ["AB", "C", "DEFG"]          # transposed
    assert tok.decode_batch_padded(x.cpu(), lengths.cpu()) == ["AB", "C", "DEFG"]   # a CPU tensor
    assert tok.decode_batch_padded(x.cpu().tolist(), [2, 1, 4]) == ["AB", "C", "DEFG"]
    assert tok.decode_batch_padded(x, lengths) == ["AB", "C", "DEFG"]           # still usable


# ---------------------------------------------------------------------- round trips
@functools.lru_cache(maxsize=None)
def _texts():
    out = []
    for name in ("tinystories_sample.txt", "german.txt"):
        out += (gpt2_files.FIXTURES / name).read_text(encoding="utf-8").splitlines(keepends=True)
    return tuple(out)


def test_round_trips():
    _, _, tok = _gpt2()
    texts = list(_texts())
    assert any("<|endoftext|>" in t for t in texts) and any(ord(c) > 127 for t in texts for c in t)
    assert tok.decode_batch(tok.encode_batch(texts)) == texts
    data, byte_off = tok.decode_batch_np(*tok.encode_batch_np(texts))
    assert [data[a:b].tobytes().decode("utf-8") for a, b in zip(byte_off[:-1], byte_off[1:])] == texts
    for side in ("right", "left"):
        rows, lengths = tok.encode_batch_padded(texts, None, pad_id=0, padding_side=side)
        assert tok.decode_batch_padded(rows, lengths, padding_side=side) == texts


def test_decode_tokens():
    _, _, tok = _gpt2()
    text = (gpt2_files.FIXTURES / "tinystories_sample.txt").read_text(encoding="utf-8")[:800]
    text += (gpt2_files.FIXTURES / "german.txt").read_text(encoding="utf-8") + " 世界 café 🙂"
    ids = tok.encode(text)[-300:]
    assert len(ids) == 300
    want = [tok.decode([i]) for i in ids]
    assert any("�" in w for w in want)    # multi-byte characters split over tokens
    assert tok.decode_tokens(ids) == want


def test_reuse_and_decode_unchanged():
    vocab, _, tok = _gpt2()
    rng = random.Random(11)
    flat = _random_ids(rng, vocab, 200_000)
    want_flat = _ref(vocab, flat)
    assert tok.decode(flat) == want_flat
    big = [flat[i:i + 997] for i in range(0, len(flat), 997)]
    first = tok.decode_batch(big)
    assert first == [_ref(vocab, r) for r in big]
    assert tok.decode_batch([[flat[0]]]) == [_ref(vocab, flat[:1])]
    assert tok.decode_batch(big) == first
    assert tok.decode(flat) == want_flat
