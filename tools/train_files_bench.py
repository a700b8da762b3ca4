"""What counting a corpus window by window, or shard by shard, costs over train_bpe(path), on one GPU.

Three ways to train on the bench's corpus (bpe_synth_corpus_host, seed 2, OWT-like, 11.9 GB, vocab
32000; page-cache warm), each timed once after one warm-up of the same call, with the device
buffers reused so that no allocation is inside the timed call (train_bpe: keep_device_buffers;
the counter: clear(), which keeps its table, pool and scratch, and the trainer's cached corpus
buffer and counter scratch):

  single    train_bpe(path)                                   existing code, the yardstick
  windowed  WordCounter.add_file(path, window_bytes) + train  (what train_bpe_files does per file)
  shards    the same bytes as --shards files cut at 4096-byte block boundaries (safe split points
            of this corpus, so the word multiset is the same), add_file each + train

All three must give the merges of tests/golden/scale/train_C3.json.gz when the corpus is that
golden's.  Each step runs in a child process under its own time limit; the first step that fails
or runs out of time ends the run (nothing is tried again).  One JSON line per step, and with
--out the lines go to that file as well.

    python tools/train_files_bench.py [--bytes 11.9e9] [--window-gib 2] [--shards 6] [--out FILE]
"""
import argparse
import ctypes
import gzip
import json
import mmap
import os
import pathlib
import subprocess
import sys
import tempfile
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "transformer-lm_amd"), str(ROOT)]

EOT = "<|endoftext|>"
BLOCK = 4096


def corpus_path(args, n):
    return pathlib.Path(args.corpus_dir) / f"bpe355_bench_s{args.seed}_f{args.flavour}_{n}.txt"


def shard_bounds(n, k):
    blocks = n // BLOCK
    cuts = [blocks * i // k * BLOCK for i in range(k)] + [n]
    return list(zip(cuts, cuts[1:]))


def shard_path(args, n, i):
    return corpus_path(args, n).with_suffix(f".shard{i}of{args.shards}")


def write_range(L, path, first_block, n, seed, flavour):
    tmp = path.with_suffix(path.suffix + ".part")
    with open(tmp, "wb+") as f:
        f.truncate(n)
        with mmap.mmap(f.fileno(), n) as m:
            buf = (ctypes.c_char * n).from_buffer(m)
            rc = L.bpe_synth_corpus_host(ctypes.addressof(buf), n, seed, flavour, first_block, 16)
            del buf
            assert rc == 0, rc
    os.replace(tmp, path)


def golden_merges(n, args):
    for p in sorted((ROOT / "tests" / "golden" / "scale").glob("train_*.json.gz")):
        g = json.load(gzip.open(p, "rt"))
        if (g["n"], g["seed"], g["flavour"], g["vocab"]) == (n, args.seed, args.flavour, args.vocab):
            return p.name, [(bytes.fromhex(a), bytes.fromhex(b)) for a, b in g["merges"]]
    return None, None


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()           # every library call returns with its stream synchronised
    return out, (time.perf_counter() - t0) * 1e3


def step(args, n):
    from bpe_amd import _lib, WordCounter, train_bpe, last_train_stats
    L = _lib.lib()
    if args.step == "write":
        t0 = time.perf_counter()
        if not corpus_path(args, n).exists():
            write_range(L, corpus_path(args, n), 0, n, args.seed, args.flavour)
        for i, (lo, hi) in enumerate(shard_bounds(n, args.shards)):
            if not shard_path(args, n, i).exists():
                write_range(L, shard_path(args, n, i), lo // BLOCK, hi - lo, args.seed, args.flavour)
        return {"seconds": round(time.perf_counter() - t0, 1)}
    _lib.require_device()
    gname, want = golden_merges(n, args)
    path = corpus_path(args, n)
    rec = {"golden": gname}
    if args.step == "single":
        train_bpe(path, args.vocab, [EOT], keep_device_buffers=True)
        (vocab, merges), ms = timed(lambda: train_bpe(path, args.vocab, [EOT], keep_device_buffers=True))
        st = last_train_stats()
    else:
        files = [path] if args.step == "windowed" else [shard_path(args, n, i) for i in range(args.shards)]
        window = int(args.window_gib * (1 << 30)) if args.step == "windowed" else None
        c = WordCounter()

        def run():
            c.clear()
            for f in files:
                c.add_file(f, window)
            t1 = time.perf_counter()
            out = c.train(args.vocab, [EOT])
            rec["train_ms"] = round((time.perf_counter() - t1) * 1e3, 1)
            return out
        run()
        (vocab, merges), ms = timed(run)
        st = last_train_stats()
        info = c.info()
        rec.update(info=info, fold_ms_per_window=round(info["t_fold_ms"] / max(1, info["n_windows"]), 2),
                   window_bytes=window, files=len(files))
        c.close()
    rec.update(total_ms=round(ms, 1), merges_equal_golden=None if want is None else merges == want,
               stats={k: st[k] for k in ("t_load_ms", "t_count_ms", "t_words_ms", "t_merge_ms", "t_total_ms",
                                         "n_bytes", "n_pretokens", "n_words")})
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=float, default=11.9e9)
    ap.add_argument("--vocab", type=int, default=32000)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--flavour", type=int, default=0)
    ap.add_argument("--window-gib", type=float, default=2.0)
    ap.add_argument("--shards", type=int, default=6)
    ap.add_argument("--corpus-dir", default=os.environ.get("BPE355_BENCH_DIR", tempfile.gettempdir()))
    ap.add_argument("--keep-corpus", action="store_true")
    ap.add_argument("--step-timeout", type=float, default=240.0, help="seconds per step")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=("write", "single", "windowed", "shards"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    n = int(args.bytes) // BLOCK * BLOCK   # whole blocks, as bench.py sizes its corpus
    if args.step:
        print(json.dumps({"step": args.step, **step(args, n)}), flush=True)
        return 0
    lines, rc = [], 0
    try:
        for name in ("write", "single", "windowed", "shards"):
            cmd = [sys.executable, os.path.abspath(__file__), "--step", name] + sys.argv[1:]
            try:
                r = subprocess.run(cmd, timeout=args.step_timeout, stdout=subprocess.PIPE, text=True)
            except subprocess.TimeoutExpired:
                print(f"[train_files_bench] step {name} passed its {args.step_timeout:.0f} s limit: stopping",
                      file=sys.stderr)
                rc = 124
                break
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            lines.append(r.stdout)
            if r.returncode != 0:
                print(f"[train_files_bench] step {name} failed ({r.returncode}): stopping", file=sys.stderr)
                rc = r.returncode
                break
    finally:
        if args.out:
            pathlib.Path(args.out).write_text("".join(lines))
        if not args.keep_corpus:
            for p in [corpus_path(args, n)] + [shard_path(args, n, i) for i in range(args.shards)]:
                if p.exists():
                    p.unlink()
    return rc


if __name__ == "__main__":
    sys.exit(main())
