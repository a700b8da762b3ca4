"""Device-to-device throughput of the UTF-8 repair (bpe_utf8_repair_device) on a synthetic text
(bpe_synth_corpus_device, OWT-like), in three states:

  clean     the text as generated (well-formed: every tile is a plain copy)
  sparse    one 0xFF byte per MiB (what a real corpus looks like: a few dirty tiles)
  all_ff    every byte 0xFF (the worst case: every byte classified, the output 3x the input)

beside bpe_text_prepare_device -- today's strict validation, which a clean window pays and nothing
more -- on the clean buffer, in the same run.  Each figure is the median of --runs timed calls
(after two warm-up calls), each call between device synchronisations on the host clock; a call is
the whole repair: classification, scan, the size read back by the host, and the write.  GB/s counts
input bytes.  replace mode; ignore writes less.

    python tools/utf8_repair_bench.py [--bytes 1073741824] [--runs 5] [--out FILE]
"""
import argparse
import ctypes
import json
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "transformer-lm_amd"), str(ROOT)]


def timed(fn, runs):
    import torch
    for _ in range(2):
        fn()
    ms = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "utf8_repair" / "utf8_repair_bench.json"))
    args = ap.parse_args()

    import torch
    from bpe_amd import _lib
    _lib.require_device()
    L = _lib.lib()
    n = args.bytes // 4096 * 4096
    clean = torch.empty(n, dtype=torch.uint8, device="cuda")
    _lib.check(L.bpe_synth_corpus_device(ctypes.c_void_p(clean.data_ptr()), n, 2, 0, 0, None), "synth")
    torch.cuda.synchronize()
    sparse = clean.clone()
    sparse[(1 << 19)::(1 << 20)] = 0xFF
    all_ff = torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda")
    out = torch.empty(3 * n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def repair(src):
        def call():
            m, st = ctypes.c_size_t(0), _lib.Utf8Stats()
            _lib.check(L.bpe_utf8_repair_device(ctypes.c_void_p(src.data_ptr()), n, 1, ctypes.c_void_p(out.data_ptr()),
                                                out.numel(), ctypes.byref(m), ctypes.byref(st), None), "repair")
            call.last = (m.value, st.n_units, st.n_bytes)
        return call

    def strict():
        m = ctypes.c_size_t(0)
        _lib.check(L.bpe_text_prepare_device(ctypes.c_void_p(clean.data_ptr()), n, ctypes.c_void_p(clean.data_ptr()),
                                             ctypes.byref(m), None), "prepare")

    res = {"bytes": n, "runs": args.runs, "mode": "replace", "device": torch.cuda.get_device_name(0), "cases": {}}
    for name, fn in (("strict_validate_clean", strict), ("repair_clean", repair(clean)),
                     ("repair_sparse", repair(sparse)), ("repair_all_ff", repair(all_ff))):
        ms = timed(fn, args.runs)
        med = statistics.median(ms)
        case = {"ms": [round(x, 3) for x in ms], "median_ms": round(med, 3), "input_GBps": round(n / med / 1e6, 1)}
        if hasattr(fn, "last"):
            case["n_out"], case["n_units"], case["n_bytes"] = fn.last
        res["cases"][name] = case
    # the calls computed what they should have
    assert res["cases"]["repair_clean"]["n_out"] == n and res["cases"]["repair_clean"]["n_units"] == 0
    sp = res["cases"]["repair_sparse"]   # (a 0xFF that lands inside a character breaks that one too)
    assert sp["n_units"] >= n >> 20 and sp["n_out"] == n - sp["n_bytes"] + 3 * sp["n_units"]
    assert res["cases"]["repair_all_ff"]["n_out"] == 3 * n
    path = pathlib.Path(args.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
