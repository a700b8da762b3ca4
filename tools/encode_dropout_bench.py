"""What encode with BPE-dropout costs, on one GPU.

Two workloads over bpe_synth_corpus_device text (OWT-like) and a 32k vocab trained on it: the
whole text as one document, and a training batch of 4096 documents of about 1 KB.  Rows, each the
median of five calls after two warm-ups, a host clock between device synchronisations:
  dropout p in {0, 0.1, 0.5}, device to device (bpe_tok_encode_dropout_device) and host to host
      (Tokenizer.encode_batch_dropout_np: UTF-8 join, copy in, encode, copy out)
  plain   the deterministic encode_batch on the same input, device to device and host to host: every
      distinct word is encoded once there, so it is a lower bound and not a target
  ref     tests/dropout_cases.py's DropoutRef (pure Python) on a 1 MB slice, p = 0.1
  hf      HF tokenizers' BPE(dropout=p) on the host, when that package imports (else no row)
One JSON line per workload.

    python tools/encode_dropout_bench.py [--bytes 64e6] [--docs 4096] [--doc-bytes 1024] [--vocab 32000]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(_ROOT, "transformer-lm_amd"), _ROOT, os.path.join(_ROOT, "tests"),
                os.path.join(_ROOT, "tests", "golden")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bpe_amd import _lib, train_bpe_device, Tokenizer  # noqa: E402

EOT = "<|endoftext|>"
PS = (0, 0.1, 0.5)
P = ctypes.c_void_p


def timed(fn, warmup, calls, device=True):
    ms = []
    for i in range(warmup + calls):
        if device:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if device:
            torch.cuda.synchronize()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "calls": len(ms)}


def hf_rows(vocab, merges, texts, n_bytes, warmup, calls):
    try:
        from tokenizers import Tokenizer as HFTokenizer, models, pre_tokenizers
    except ImportError:
        return None
    import gpt2_files
    enc = gpt2_files.byte_to_printable()
    s = lambda b: "".join(enc[x] for x in b)   # noqa: E731
    hv = {s(b): i for i, b in vocab.items()}
    hm = [(s(a), s(b)) for a, b in merges]
    rows = {}
    for p in PS:
        tk = HFTokenizer(models.BPE(vocab=hv, merges=hm, dropout=float(p) if p else None))
        tk.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=True)
        r = timed(lambda: tk.encode_batch(texts), warmup, calls, device=False)
        r["MB_per_s"] = round(n_bytes / r["median_ms"] / 1e3, 1)
        rows[f"p={p}"] = r
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=float, default=64e6)
    ap.add_argument("--docs", type=int, default=4096)
    ap.add_argument("--doc-bytes", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--vocab", type=int, default=32000)
    ap.add_argument("--ref-bytes", type=int, default=1_000_000)
    ap.add_argument("--no-hf", action="store_true")
    args = ap.parse_args()
    L = _lib.lib()
    _lib.require_device()
    n = max(1, int(args.bytes) // 4096) * 4096
    text = torch.empty(n, dtype=torch.uint8, device="cuda")
    _lib.check(L.bpe_synth_corpus_device(P(text.data_ptr()), n, 2, 0, 0, None), "synth")
    torch.cuda.synchronize()
    vocab, merges = train_bpe_device(text.data_ptr(), n, args.vocab, [EOT])
    tok = Tokenizer(vocab, merges, [EOT])
    h = tok._device()
    host = bytes(text.cpu().numpy())
    k = ctypes.c_size_t(0)

    # the documents of the batch workload end at spaces, so that each is valid UTF-8 text of its own
    docs, a = [], 0
    while len(docs) < args.docs and a + args.doc_bytes < n:
        b = host.find(b" ", a + args.doc_bytes - 32)
        b = n if b < 0 else b
        docs.append(host[a:b].decode("utf-8"))
        a = b
    workloads = [("one document", [host.decode("utf-8")]), (f"{len(docs)} documents", docs)]

    for name, texts in workloads:
        data, starts = tok._join(texts)
        m, nd = len(data), len(texts)
        d_text = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        ids = torch.empty(m, dtype=torch.int32, device="cuda")
        offs = torch.empty(nd + 1, dtype=torch.int64, device="cuda")
        out = {"what": "encode with dropout", "workload": name, "bytes": m, "docs": nd, "vocab": len(vocab),
               "method": f"median of {args.calls} after {args.warmup} warm-ups, host clock between device synchronisations"}

        def dropout_dev(thr):
            _lib.check(L.bpe_tok_encode_dropout_device(h, P(d_text.data_ptr()), m, starts.ctypes.data, nd, thr, 7, 0,
                                                       P(ids.data_ptr()), ctypes.byref(k), P(offs.data_ptr()), None),
                       "dropout")

        def plain_dev():
            _lib.check(L.bpe_tok_encode_batch_device(h, P(d_text.data_ptr()), m, starts.ctypes.data, nd,
                                                     P(ids.data_ptr()), ctypes.byref(k), P(offs.data_ptr()), None), "batch")

        rows = {}
        r = timed(plain_dev, args.warmup, args.calls)
        r["ids"] = k.value
        plain_ids = ids[:k.value].clone()
        rows["plain device"] = r
        rows["plain host"] = timed(lambda: tok.encode_batch_np(texts), args.warmup, args.calls)
        for p in PS:
            thr = int(round(p * 2 ** 24))
            r = timed(lambda: dropout_dev(thr), args.warmup, args.calls)
            r["ids"] = k.value
            if p == 0:
                assert torch.equal(ids[:k.value], plain_ids), "p = 0 differs from the deterministic encode"
            rows[f"dropout p={p} device"] = r
            rows[f"dropout p={p} host"] = timed(lambda: tok.encode_batch_dropout_np(texts, p, 7), args.warmup, args.calls)
        for r in rows.values():
            r["MB_per_s"] = round(m / r["median_ms"] / 1e3, 1)
        out["rows"] = rows
        if name == "one document":
            import dropout_cases as dc
            ref = dc.DropoutRef(vocab, merges, [EOT])
            cut = host.rfind(b" ", 0, args.ref_bytes)
            piece = host[:cut].decode("utf-8")
            t0 = time.perf_counter()
            want = ref.encode_dropout(piece, 0.1, 7)
            sec = time.perf_counter() - t0
            assert tok.encode_dropout(piece, 0.1, 7) == want, "the device path differs from DropoutRef"
            out["ref"] = {"bytes": cut, "p": 0.1, "seconds": round(sec, 3), "MB_per_s": round(cut / sec / 1e6, 3),
                          "matches_device": True}
        if not args.no_hf:
            hf = hf_rows(vocab, merges, texts, m, 1, 3) if name != "one document" else None
            out["hf_tokenizers"] = hf if hf is not None else "not measured (the package does not import, or one-document workload)"
        print(json.dumps(out), flush=True)
        del d_text, ids, offs


if __name__ == "__main__":
    main()
