"""GPU: the device pre-tokenizer's character classes over every Unicode scalar value, against the
C oracle (pinned to the `regex` module on the CPU by tests/test_unicode_classes.py; `regex` itself
is not needed here).  The texts are those of tests/unicode_cases.py.

The device classifies a code point on three paths, and these tests reach each with all of them:

  * context texts (each scalar value between letters, digits, punctuation and before "'s"): every
    pre-token is short, so the token starts come from the byte-parallel predicate -- the LDS table
    g_cls2 below U+0800 (csrc/stage2.h) and uc_class<DevTab> on the paged global tables above
    (csrc/tokstart.h) -- in the counter (word counts, train) and in the encoder's scan;
  * class-run texts (one pre-token per class and plane, up to 262 KB) and the serial-scanner text
    (runs of 2.25 KiB, each the last pre-token that starts in its 16 KiB chunk and ending more
    than the 1 KiB halo past it): the end of such a pre-token is found by token_end/class_at
    (csrc/pretok.h), on the staged window and then on global memory;
  * a device pointer shifted by 1 and by 7 bytes: the byte-wise staging path in front of both.

The encoder runs with the 256 byte tokens plus one merge per byte pair, ranked so that an ASCII
byte merges with a neighbouring character exactly when no pre-token boundary lies between them.

Measured on an MI355X: the 56 tests take 12 s together; every test takes 0.3 s or less, oracle
included, but test_encode_serial_scanner: oracle 0.3 s, device 2.0 s.  Both are quadratic in the
pre-token length with this tokenizer (every pair merges).  With runs of 16 KiB the oracle alone took
9.1 s on the build machine (8 KiB: 5.9 s), and with runs of 4 KiB the device took 4.7 s (oracle
0.4 s), so the run length was halved until neither side comes near 5 s: 2304 bytes, still more
than twice the halo, and every run still ends past its chunk's staged window.
"""
from __future__ import annotations

import pytest

import unicode_cases as U
from oracle import oracle

pytestmark = pytest.mark.gpu

bpe_amd = pytest.importorskip("bpe_amd")
from test_gpu_utf8 import _device_word_counts  # noqa: E402

SERIAL_RUN_BYTES = 2304


@pytest.fixture(scope="module", autouse=True)
def _device():
    from bpe_amd import _lib
    _lib.require_device()


@pytest.fixture(scope="module")
def tokenizer():
    vocab, merges = U.all_pairs_tokenizer()
    tok = bpe_amd.Tokenizer(dict(vocab), list(merges), [])
    yield tok
    tok.release_device_buffers()


def _check_words(text: str):
    data = text.encode("utf-8")
    want = {w: c for w, c in oracle.word_counts(data, []).items() if len(w) > 1}
    got = _device_word_counts(data, [])
    if got != want:
        diff = sorted(set(got.items()) ^ set(want.items()), key=lambda kv: (len(kv[0]), kv[0]))
        pytest.fail(f"{len(diff)} word-table entries differ, e.g. "
                    f"{[(w[:40].decode('utf-8', 'replace'), len(w), c) for w, c in diff[:4]]!r}")


def _check_encode(tok, text: str):
    vocab, merges = U.all_pairs_tokenizer()
    want = oracle.encode(vocab, merges, [], text)
    got = tok.encode(text)
    if got != want:
        i = next((k for k, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        pytest.fail(f"ids differ at index {i} of {len(got)} / {len(want)}: device {got[i:i + 6]}, "
                    f"oracle {want[i:i + 6]} ({[vocab[t] for t in want[i:i + 6]]!r})")


@pytest.mark.parametrize("plane", U.PLANES)
def test_word_counts_context_text(plane):
    _check_words(U.context_text(plane))


@pytest.mark.parametrize("plane", U.PLANES)
def test_word_counts_class_runs(plane):
    _check_words(U.class_run_text(plane))


@pytest.mark.parametrize("shift", [1, 7])
def test_train_unaligned_pointer(shift):
    import torch
    data = U.context_text(0).encode("utf-8")
    buf = torch.zeros(len(data) + 16, dtype=torch.uint8, device="cuda")
    buf[shift:shift + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    got = bpe_amd.train_bpe_device(buf.data_ptr() + shift, len(data), 300, [])
    assert got == oracle.train_raw(data, 300, [])


@pytest.mark.parametrize("plane", U.PLANES)
def test_encode_context_text(tokenizer, plane):
    _check_encode(tokenizer, U.context_text(plane))


@pytest.mark.parametrize("knob", ["BPE355_NOCACHE=1", "BPE355_ENC_PEND_CAP=0"])
def test_encode_context_text_variants(tokenizer, knob, monkeypatch):
    """no LDS word cache (every word goes to the pending pool); no pending pool (the scan resolves
    every word itself)"""
    monkeypatch.setenv(*knob.split("="))
    _check_encode(tokenizer, U.context_text(0))


def test_encode_serial_scanner(tokenizer):
    text, spans = U.serial_scanner_text(SERIAL_RUN_BYTES)
    assert len(spans) > 40 and min(n for _s, n in spans) > 2 * U.K_HALO
    # every run ends past its chunk's staged window: token_end's global-memory fallback
    assert all(s + n > (s // U.K_CHUNK + 1) * U.K_CHUNK + U.K_HALO for s, n in spans)
    _check_encode(tokenizer, text)
