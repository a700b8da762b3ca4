"""What the spans of encode-with-offsets cost, on one GPU.

1 GiB of bpe_synth_corpus_device text in HBM, a 32k vocab trained on it, document starts every
4096 bytes and (a second run) every 128 bytes.  bpe_tok_encode_spans_device with unit byte and with
unit char is timed against bpe_tok_encode_batch_device on the same text and starts -- the batch call
is the span call without the spans, so the difference is their price -- the three alternating, a
host clock around calls that end in a stream synchronise.  Median and min..max over the timed
calls, one JSON line per configuration.  (Starts at fixed byte steps cut characters; that changes
nothing the kernels do.)

    python tools/encode_spans_bench.py [--bytes N] [--calls 7] [--warmup 2] [--vocab 32000] [--doc-bytes 4096,128]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(_ROOT, "transformer-lm_amd"), _ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bpe_amd import _lib, train_bpe_device, Tokenizer  # noqa: E402

EOT = "<|endoftext|>"


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "calls": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=float, default=float(1 << 30))
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--vocab", type=int, default=32000)
    ap.add_argument("--doc-bytes", default="4096,128", help="bytes between document starts, one run each")
    args = ap.parse_args()
    assert args.calls >= 5, "at least 5 timed calls"
    L = _lib.lib()
    _lib.require_device()
    n = max(1, int(args.bytes) // 4096) * 4096
    P = ctypes.c_void_p
    text = torch.empty(n, dtype=torch.uint8, device="cuda")
    _lib.check(L.bpe_synth_corpus_device(P(text.data_ptr()), n, 2, 0, 0, None), "synth")
    torch.cuda.synchronize()
    vocab, merges = train_bpe_device(text.data_ptr(), n, args.vocab, [EOT])
    tok = Tokenizer(vocab, merges, [EOT])
    h = tok._device()
    ids = torch.empty(n, dtype=torch.int32, device="cuda")
    ids2 = torch.empty(n, dtype=torch.int32, device="cuda")
    spans = torch.empty((n, 2), dtype=torch.int32, device="cuda")
    k = ctypes.c_size_t(0)

    for step in [int(x) for x in args.doc_bytes.split(",")]:
        starts = np.arange(0, n, step, dtype=np.uint64)
        nd = len(starts)
        offs = torch.empty(nd + 1, dtype=torch.int64, device="cuda")
        offs2 = torch.empty(nd + 1, dtype=torch.int64, device="cuda")

        def batch():
            _lib.check(L.bpe_tok_encode_batch_device(h, P(text.data_ptr()), n, starts.ctypes.data, nd,
                                                     P(ids2.data_ptr()), ctypes.byref(k), P(offs2.data_ptr()), None),
                       "batch")

        def with_spans(unit):
            _lib.check(L.bpe_tok_encode_spans_device(h, P(text.data_ptr()), n, starts.ctypes.data, nd, unit,
                                                     P(ids.data_ptr()), ctypes.byref(k), P(offs.data_ptr()),
                                                     P(spans.data_ptr()), None), "spans")

        t = {"batch": [], "spans_byte": [], "spans_char": []}
        byte_spans = None
        for i in range(args.warmup + args.calls):
            for name, fn in (("batch", batch), ("spans_byte", lambda: with_spans(0)),
                             ("spans_char", lambda: with_spans(1))):   # alternating: the same machine state
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()                      # ends in a stream synchronise
                ms = (time.perf_counter() - t0) * 1e3
                if i >= args.warmup:
                    t[name].append(ms)
                if i == 0 and name == "spans_byte":
                    byte_spans = spans[:k.value].clone()
        m = k.value
        # the calls computed the same ids and offsets; the byte spans are ordered inside a document
        assert torch.equal(ids[:m], ids2[:m]) and torch.equal(offs, offs2), "span and batch results differ"
        assert bool((byte_spans[:, 0] < byte_spans[:, 1]).all())
        b, sb, sc = summary(t["batch"]), summary(t["spans_byte"]), summary(t["spans_char"])
        print(json.dumps({"what": "encode_spans vs encode_batch", "bytes": n, "doc_bytes": step, "docs": nd, "ids": m,
                          "batch": b, "spans_byte": sb, "spans_char": sc,
                          "byte_cost_ms": round(sb["median_ms"] - b["median_ms"], 3),
                          "byte_cost_pct": round(100 * (sb["median_ms"] / b["median_ms"] - 1), 2),
                          "char_cost_ms": round(sc["median_ms"] - b["median_ms"], 3),
                          "char_cost_pct": round(100 * (sc["median_ms"] / b["median_ms"] - 1), 2)}), flush=True)
        del offs, offs2, byte_spans


if __name__ == "__main__":
    main()
