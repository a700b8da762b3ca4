"""What the batch encode's id offsets cost, and the padded-rows kernel, on one GPU.

1 GiB of bpe_synth_corpus_device text in HBM, a 32k vocab trained on it, document starts every
4096 bytes and (a second run) every 128 bytes.  bpe_tok_encode_batch_device is timed against
bpe_tok_encode_chunks_device on the same text and starts -- the chunks call is the encoder without
the offsets, so the difference is their price -- the two alternating, a host clock around calls
that end in a stream synchronise.  k_pack_rows (bpe_ids_pack_rows_device) is timed at T = 512 by
device events.  Median and min..max over the timed calls, one JSON line per configuration.

    python tools/encode_batch_bench.py [--bytes N] [--calls 7] [--warmup 2] [--vocab 32000] [--doc-bytes 4096,128]
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
    k = ctypes.c_size_t(0)

    for step in [int(x) for x in args.doc_bytes.split(",")]:
        starts = np.arange(0, n, step, dtype=np.uint64)
        nd = len(starts)
        offs = torch.empty(nd + 1, dtype=torch.int64, device="cuda")

        def chunks():
            _lib.check(L.bpe_tok_encode_chunks_device(h, P(text.data_ptr()), n, starts.ctypes.data, nd,
                                                      P(ids2.data_ptr()), ctypes.byref(k), None), "chunks")

        def batch():
            _lib.check(L.bpe_tok_encode_batch_device(h, P(text.data_ptr()), n, starts.ctypes.data, nd,
                                                     P(ids.data_ptr()), ctypes.byref(k), P(offs.data_ptr()), None),
                       "batch")

        t = {"chunks": [], "batch": []}
        for i in range(args.warmup + args.calls):
            for name, fn in (("chunks", chunks), ("batch", batch)):   # alternating: the same machine state
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()                      # ends in a stream synchronise
                ms = (time.perf_counter() - t0) * 1e3
                if i >= args.warmup:
                    t[name].append(ms)
        m = k.value
        # the two calls computed the same ids, and the offsets close the id stream
        assert torch.equal(ids[:m], ids2[:m]), "batch and chunks ids differ"
        o = offs.cpu().numpy()
        assert o[0] == 0 and o[-1] == m and (np.diff(o) >= 0).all()
        c, b = summary(t["chunks"]), summary(t["batch"])

        # padded rows at T = 512, device events around the call
        T = 512
        for dtype in (torch.int32, torch.int64):
            out = torch.empty((nd, T), dtype=dtype, device="cuda")
            lengths = torch.empty(nd, dtype=torch.int32, device="cuda")
            ev = []
            for i in range(args.warmup + args.calls):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _lib.check(L.bpe_ids_pack_rows_device(P(ids.data_ptr()), P(offs.data_ptr()), nd, T, 0, 0,
                                                      out.element_size(), P(out.data_ptr()), P(lengths.data_ptr()),
                                                      P(torch.cuda.current_stream().cuda_stream)), "pack rows")
                e1.record()
                e1.synchronize()
                if i >= args.warmup:
                    ev.append(e0.elapsed_time(e1))
            p = summary(ev)
            p["GBps_written"] = round(out.numel() * out.element_size() / (p["median_ms"] * 1e-3) / 1e9, 1)
            print(json.dumps({"what": "k_pack_rows", "rows": nd, "T": T, "dtype": str(dtype).split(".")[1],
                              "kept_ids": int(lengths.sum().item()), **p}), flush=True)
            del out, lengths
        print(json.dumps({"what": "encode_batch vs encode_chunks", "bytes": n, "doc_bytes": step, "docs": nd, "ids": m,
                          "chunks": c, "batch": b,
                          "offsets_cost_ms": round(b["median_ms"] - c["median_ms"], 3),
                          "offsets_cost_pct": round(100 * (b["median_ms"] / c["median_ms"] - 1), 2)}), flush=True)
        del offs


if __name__ == "__main__":
    main()
