"""What one batch costs per call, at the reference's default batch size B = 128, for T = 256 and
T = 1024, on one GPU, from a synthetic uint16 token file with separators (GPT-2 sized ids, documents
of about 600 ids; written with NumPy from a seed, page-cache warm):

  ref_loop      the reference's way on np.memmap, restated: torch.randint starts, a Python loop of
                slices into two float64 arrays, two torch.tensor(..., long, device) copies
  load_batch    bpe_amd.batches.load_batch on the same memmap (the drop-in: staging path)
  host_batch    TokenStore.from_array(memmap).sample, the same path without the int64 requirement
  sample        TokenStore.sample on a resident store, int64
  sample_docs   the same with positions, doc_ids and ignore_index
  torch         what a user would write on the resident tensor: ids[starts[:, None] + arange(T + 1)]
                .long() and two slices
  torch_docs    the same plus positions and doc_ids by torch.searchsorted on the index and targets
                masked with torch.where

Every timing is a window of many calls (sized to about --window seconds after a warm-up of the same
shape) between two device synchronisations; --runs windows, the median per call is reported.  The
starts are drawn inside the call in every variant, as a training loop would.  Before anything is
timed, sample/batch is held against the torch expression at the same starts.

    python tools/load_batch_bench.py [--ids 1e8] [--runs 5] [--out FILE]
"""
import argparse
import json
import os
import pathlib
import statistics
import sys
import tempfile
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "transformer-lm_amd"), str(ROOT)]

SEP = 50256
B = 128


def write_tokens(path, idx_path, n, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, SEP, n, dtype=np.uint16)
    ends = np.cumsum(rng.geometric(1.0 / 600.0, int(n / 600 * 1.2) + 16))
    ends = ends[ends < n]
    ids[ends] = SEP
    ids.tofile(path)
    np.flatnonzero(ids == SEP).astype(np.uint64).tofile(idx_path)


def per_call(fn, window_s, runs):
    """Median microseconds per call over `runs` windows of about window_s seconds."""
    import torch
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    each = (time.perf_counter() - t0) / 20
    calls = int(min(20000, max(20, window_s / max(each, 1e-7))))
    us = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        us.append(round((time.perf_counter() - t0) / calls * 1e6, 2))
    return {"calls_per_window": calls, "us": us, "median_us": statistics.median(us), "min_us": min(us),
            "max_us": max(us)}


def ref_loop(dataset, batch_size, context_length, device):
    """The reference's load_batch, restated (models/util.py:37-57)."""
    import numpy as np
    import torch
    x = np.zeros((batch_size, context_length))
    y = np.zeros((batch_size, context_length))
    first = torch.randint(len(dataset) - context_length, (batch_size,))
    for r, s in enumerate(first):
        x[r] = dataset[s:s + context_length]
        y[r] = dataset[s + 1:s + context_length + 1]
    return (torch.tensor(x, dtype=torch.long, device=device), torch.tensor(y, dtype=torch.long, device=device))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ids", type=float, default=1e8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds per timing window")
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--dir", default=os.environ.get("BPE355_BENCH_DIR", tempfile.gettempdir()))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    from bpe_amd import _lib
    from bpe_amd.batches import TokenStore, load_batch
    _lib.require_device()
    n = int(args.ids)
    path = pathlib.Path(args.dir) / f"bpe355_load_batch_{args.seed}_{n}.bin"
    idx_path = path.with_suffix(".idx")
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line + "\n")

    try:
        write_tokens(path, idx_path, n, args.seed)
        mm = np.memmap(path, dtype=np.uint16, mode="r")
        dev = torch.device("cuda", torch.cuda.current_device())
        t0 = time.perf_counter()
        store = TokenStore.from_file(path, np.uint16, index_path=idx_path, separator_id=SEP)
        torch.cuda.synchronize()
        open_ms = round((time.perf_counter() - t0) * 1e3, 1)
        host = TokenStore.from_array(mm, device=dev)
        ids = torch.from_numpy(np.fromfile(path, dtype=np.int16)).to(dev).view(torch.uint16)
        sep = torch.from_numpy(np.fromfile(idx_path, dtype=np.uint64).view(np.int64)).to(dev)
        try:   # indexing uint16 on the device, where this torch has it; else the int16 bits, masked
            ids[torch.zeros(2, dtype=torch.int64, device=dev)].long()
            variant = "uint16 index"

            def windows(idx):
                return ids[idx].long()
        except RuntimeError:
            variant = "int16 index, & 0xFFFF"
            bits = ids.view(torch.int16)

            def windows(idx):
                return bits[idx].long() & 0xFFFF
        emit({"step": "open", "n_ids": n, "n_docs": store.n_docs, "from_file_ms": open_ms,
              "device_bytes": store.device_bytes, "torch_variant": variant, "batch_size": B})

        for T in (256, 1024):
            ar1 = torch.arange(T + 1, device=dev)
            ar = ar1[:T]

            def torch_plain(starts=None):
                s = torch.randint(n - T, (B,), device=dev) if starts is None else starts
                w = windows(s[:, None] + ar1)
                return w[:, :-1], w[:, 1:], s

            def torch_docs(starts=None):
                x, y, s = torch_plain(starts)
                g = s[:, None] + ar
                k = torch.searchsorted(sep, g)
                last = torch.where(k > 0, sep[(k - 1).clamp_(min=0)], -1)
                return x, torch.where(x == SEP, -100, y), g - last - 1, (k - k[:, :1]).int(), s

            # the same numbers from both, before anything is timed
            s = torch.randint(n - T, (B,), device=dev)
            got = store.batch(s, T, positions=True, doc_ids=True, ignore_index=-100)
            want = torch_docs(s)
            equal = all(bool(torch.equal(a, b)) for a, b in zip(got[:4], want[:4]))
            plain = store.batch(s, T)
            equal = equal and bool(torch.equal(plain.targets, torch_plain(s)[1]))
            hb = host.batch(s.cpu(), T)
            equal = equal and bool(torch.equal(hb.inputs, plain.inputs)) and bool(torch.equal(hb.targets, plain.targets))
            rec = {"step": "time", "T": T, "batch_size": B, "equal": equal}
            if not equal:
                emit(rec)
                return 1
            rec["ref_loop"] = per_call(lambda: ref_loop(mm, B, T, dev), args.window, args.runs)
            rec["load_batch"] = per_call(lambda: load_batch(mm, B, T, dev), args.window, args.runs)
            rec["host_batch"] = per_call(lambda: host.sample(B, T), args.window, args.runs)
            rec["sample"] = per_call(lambda: store.sample(B, T), args.window, args.runs)
            rec["sample_docs"] = per_call(lambda: store.sample(B, T, positions=True, doc_ids=True, ignore_index=-100),
                                          args.window, args.runs)
            rec["torch"] = per_call(torch_plain, args.window, args.runs)
            rec["torch_docs"] = per_call(torch_docs, args.window, args.runs)
            emit(rec)
    finally:
        for p in (path, idx_path):
            if p.exists():
                p.unlink()
        if args.out:
            pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            pathlib.Path(args.out).write_text("".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
