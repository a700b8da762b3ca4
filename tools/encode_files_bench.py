"""What the dataset encoder bpe_amd.encode_files costs against the existing bulk path, on one GPU.

On a synthetic corpus (bpe_synth_corpus_host, seed 2, OWT-like; page-cache warm) encoded with the
GPT-2 tokenizer of tests/golden/fixtures, each of these is run once to warm up (device buffers
kept, so that no allocation is inside a timed call) and then --runs times:

  parent       encode_file(tok, path, out, fmt="bin")     existing code with its tofile, the yardstick
  files        encode_files(tok, [path], out)             default window
  files_stats  the same with separator=<|endoftext|>, index_path and count_ids
  id_counts    bpe_amd.id_counts on the whole uint16 id stream in HBM
  bincount     torch.bincount on the same stream (after the int64 up-conversion it needs, which is
               timed with it)

The token file of `files` must equal the parent's byte for byte, the index np.flatnonzero and the
counts np.bincount of it.  The steps run in a child process under a time limit; the first step
that fails or runs out of time ends the run (nothing is tried again).  One JSON line per step, and
with --out the lines go to that file as well.

    python tools/encode_files_bench.py [--bytes 2e9] [--runs 5] [--out FILE]
"""
import argparse
import ctypes
import json
import mmap
import os
import pathlib
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "transformer-lm_amd"), str(ROOT), str(ROOT / "tests")]

EOT = "<|endoftext|>"
BLOCK = 4096


def corpus_path(args, n):
    return pathlib.Path(args.corpus_dir) / f"bpe355_bench_s{args.seed}_f{args.flavour}_{n}.txt"


def write_corpus(L, path, n, seed, flavour):
    tmp = path.with_suffix(path.suffix + ".part")
    with open(tmp, "wb+") as f:
        f.truncate(n)
        with mmap.mmap(f.fileno(), n) as m:
            buf = (ctypes.c_char * n).from_buffer(m)
            rc = L.bpe_synth_corpus_host(ctypes.addressof(buf), n, seed, flavour, 0, 16)
            del buf
            assert rc == 0, rc
    os.replace(tmp, path)


def runs_of(fn, k):
    import torch
    fn()   # warm-up
    ms = []
    for _ in range(k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(round((time.perf_counter() - t0) * 1e3, 2))
    return {"ms": ms, "median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def step(args, n):
    import numpy as np
    from bpe_amd import _lib
    L = _lib.lib()
    path = corpus_path(args, n)
    if args.step == "write":
        t0 = time.perf_counter()
        if not path.exists():
            write_corpus(L, path, n, args.seed, args.flavour)
        return {"seconds": round(time.perf_counter() - t0, 1)}
    import torch
    import bpe_amd
    import gpt2_files
    from bpe_amd.encode import encode_file
    _lib.require_device()
    vocab, merges = gpt2_files.load_gpt2([EOT])
    tok = bpe_amd.Tokenizer(dict(vocab), list(merges), [EOT])
    out_parent = path.with_suffix(".parent.bin")
    out_files = path.with_suffix(".files.bin")
    out_idx = path.with_suffix(".files.idx")
    rec = {"bytes": n, "runs": args.runs}
    last = {}
    try:
        rec["parent"] = runs_of(lambda: encode_file(tok, path, out_parent, fmt="bin", keep_device_buffers=True),
                                args.runs)
        tok.release_device_buffers()

        def files(**kw):
            last.update(bpe_amd.encode_files(tok, [path], out_files, keep_device_buffers=True, **kw))
        rec["files"] = runs_of(files, args.runs)
        ids = np.fromfile(out_files, np.uint16)
        rec["files"]["equal_parent"] = bool(np.array_equal(ids, np.fromfile(out_parent, np.uint16)))
        rec["files"]["phases_ms"] = {k: round(last[k], 1) for k in ("read_ms", "decode_ms", "encode_ms", "write_ms")}
        rec["files"]["device_bytes"] = int(last["device_bytes"])
        rec["files_stats"] = runs_of(lambda: files(separator=EOT, index_path=out_idx, count_ids=True), args.runs)
        sep = tok.vocab_inv[EOT.encode()]
        rec["files_stats"]["index_equal"] = bool(np.array_equal(np.fromfile(out_idx, np.uint64),
                                                                np.flatnonzero(ids == sep)))
        rec["files_stats"]["counts_equal"] = bool(np.array_equal(
            last["id_counts"], np.bincount(ids, minlength=last["id_counts"].size).astype(np.uint64)))
        rec["files_stats"]["stats_ms"] = round(last["stats_ms"], 1)
        rec.update(n_ids=int(last["n_ids"]), n_windows=int(last["n_windows"]), n_separators=int(last["n_separators"]))
        tok.release_device_buffers()
        d = torch.from_numpy(ids.view(np.int16)).cuda().view(torch.uint16)
        size = max(tok.vocab) + 1
        rec["id_counts"] = runs_of(lambda: bpe_amd.id_counts(d, size), args.runs)
        rec["bincount"] = runs_of(lambda: torch.bincount(d.to(torch.int64), minlength=size), args.runs)
        rec["id_positions"] = runs_of(lambda: bpe_amd.id_positions(d, sep), args.runs)
    finally:
        for p in (out_parent, out_files, out_idx):
            if p.exists():
                p.unlink()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=float, default=2e9)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--flavour", type=int, default=0)
    ap.add_argument("--corpus-dir", default=os.environ.get("BPE355_BENCH_DIR", tempfile.gettempdir()))
    ap.add_argument("--keep-corpus", action="store_true")
    ap.add_argument("--step-timeout", type=float, default=300.0, help="seconds per step")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=("write", "encode"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    n = int(args.bytes) // BLOCK * BLOCK
    if args.step:
        print(json.dumps({"step": args.step, **step(args, n)}), flush=True)
        return 0
    lines, rc = [], 0
    try:
        for name in ("write", "encode"):
            cmd = [sys.executable, os.path.abspath(__file__), "--step", name] + sys.argv[1:]
            try:
                r = subprocess.run(cmd, timeout=args.step_timeout, stdout=subprocess.PIPE, text=True)
            except subprocess.TimeoutExpired:
                print(f"[encode_files_bench] step {name} passed its {args.step_timeout:.0f} s limit: stopping",
                      file=sys.stderr)
                rc = 124
                break
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            lines.append(r.stdout)
            if r.returncode != 0:
                print(f"[encode_files_bench] step {name} failed ({r.returncode}): stopping", file=sys.stderr)
                rc = r.returncode
                break
    finally:
        if args.out:
            pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            pathlib.Path(args.out).write_text("".join(lines))
        if not args.keep_corpus and corpus_path(args, n).exists():
            corpus_path(args, n).unlink()
    return rc


if __name__ == "__main__":
    sys.exit(main())
