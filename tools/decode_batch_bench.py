"""What the batch decode saves over a loop of decode(), and the tiled gather against the per-id
gather, on one GPU.  GPT-2 fixture vocab; the ids are the fixture texts encoded, repeated.

(a) rows: a Python loop of Tokenizer.decode(row) -- unchanged by the batch decode, so the cost
    before it -- against one Tokenizer.decode_batch(rows), the two alternating, a host clock around
    calls that end in a stream synchronise.  A generation-like shape (64 rows x 256 ids) and a
    token-like one (4096 rows x 1 id).
(b) gather: bpe_dec_decode_batch_device (k_dec_gather_tiled) against the unchanged
    bpe_dec_decode_device (k_dec_gather) on the same 16 M flat ids in device memory, alternating,
    device events around each call on one stream.  Both calls run k_dec_len and a scan in front of
    their gather; the old call allocates its arrays inside the timed window, as it always does.  For
    the gather kernels alone, run `--only gather` under `rocprofv3 --kernel-trace --stats`.

Median and min..max over the timed calls, one JSON line per configuration.

    python tools/decode_batch_bench.py [--calls 7] [--warmup 2] [--ids 16777216] [--only rows|gather]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(_ROOT, "transformer-lm_amd"), os.path.join(_ROOT, "tests"), _ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gpt2_files  # noqa: E402
from bpe_amd import _lib, Tokenizer  # noqa: E402

EOT = "<|endoftext|>"
P = ctypes.c_void_p


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "calls": len(ms)}


def fixture_ids(tok, n):
    text = "".join((gpt2_files.FIXTURES / f).read_text(encoding="utf-8")
                   for f in ("tinystories_sample.txt", "corpus.en", "german.txt"))
    ids = np.array(tok.encode(text), dtype=np.uint32)
    return np.tile(ids, n // ids.size + 1)[:n]


def bench_rows(tok, args):
    for n_rows, row_len in ((64, 256), (4096, 1)):
        flat = fixture_ids(tok, n_rows * row_len).tolist()
        rows = [flat[i * row_len:(i + 1) * row_len] for i in range(n_rows)]
        want = [tok.decode(r) for r in rows]
        assert tok.decode_batch(rows) == want
        t = {"loop": [], "batch": []}
        for i in range(args.warmup + args.calls):
            for name, fn in (("loop", lambda: [tok.decode(r) for r in rows]), ("batch", lambda: tok.decode_batch(rows))):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()                      # every library call ends in a stream synchronise
                ms = (time.perf_counter() - t0) * 1e3
                if i >= args.warmup:
                    t[name].append(ms)
        a, b = summary(t["loop"]), summary(t["batch"])
        print(json.dumps({"what": "decode() loop vs decode_batch", "rows": n_rows, "ids_per_row": row_len,
                          "bytes": sum(len(w.encode("utf-8")) for w in want), "loop": a, "batch": b,
                          "speedup": round(a["median_ms"] / b["median_ms"], 1)}), flush=True)


def bench_gather(tok, args):
    L = _lib.lib()
    dec = tok._decoder()
    n = args.ids
    ids = fixture_ids(tok, n)
    total = int(np.array([len(tok.vocab[i]) for i in range(len(tok.vocab))], dtype=np.int64)[ids].sum())
    d_ids = torch.from_numpy(ids.view(np.int32)).cuda()
    d_off = torch.tensor([0, n], dtype=torch.int64, device="cuda")
    d_byte_off = torch.empty(2, dtype=torch.int64, device="cuda")
    out_old = torch.empty(total, dtype=torch.uint8, device="cuda")
    out_new = torch.empty(total, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    sp = P(stream.cuda_stream)
    k = ctypes.c_size_t(0)

    def old():
        _lib.check(L.bpe_dec_decode_device(dec, P(d_ids.data_ptr()), n, P(out_old.data_ptr()), total, ctypes.byref(k),
                                           sp), "decode_device")

    def new():
        _lib.check(L.bpe_dec_decode_batch_device(dec, P(d_ids.data_ptr()), n, P(d_off.data_ptr()), 1,
                                                 P(out_new.data_ptr()), total, ctypes.byref(k), P(d_byte_off.data_ptr()),
                                                 None, sp), "decode_batch_device")

    t = {"per_id": [], "tiled": []}
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for i in range(args.warmup + args.calls):
            for name, fn in (("per_id", old), ("tiled", new)):   # alternating: the same machine state
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                assert k.value == total
                if i >= args.warmup:
                    t[name].append(e0.elapsed_time(e1))
    torch.cuda.synchronize()
    assert torch.equal(out_old, out_new), "the two gathers differ"
    a, b = summary(t["per_id"]), summary(t["tiled"])
    print(json.dumps({"what": "bpe_dec_decode_device (per-id gather) vs bpe_dec_decode_batch_device (tiled gather)",
                      "ids": n, "bytes": total, "per_id": a, "tiled": b,
                      "tiled_over_per_id": round(b["median_ms"] / a["median_ms"], 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ids", type=int, default=1 << 24)
    ap.add_argument("--only", choices=("rows", "gather"))
    args = ap.parse_args()
    assert args.calls >= 5, "at least 5 timed calls"
    _lib.lib()
    _lib.require_device()
    vocab, merges = gpt2_files.load_gpt2([EOT])
    tok = Tokenizer(dict(vocab), list(merges), [EOT])
    if args.only != "gather":
        bench_rows(tok, args)
    if args.only != "rows":
        bench_gather(tok, args)


if __name__ == "__main__":
    main()
