"""Ill-formed UTF-8: the errors= keyword of every entry point that reads text.

errors is "strict" (the default: UnicodeDecodeError, as the reference), "replace" or "ignore", with
CPython's meaning: bytes.decode("utf-8", errors).  The repair runs on the device
(csrc/utf8fix.hip) and only after the strict validation of a window has failed, so clean input
pays nothing.
"""
from __future__ import annotations

import ctypes

from . import _lib

__all__ = ["repair_utf8", "last_utf8_errors", "repair_geometry"]

_MODES = {"strict": 0, "replace": 1, "ignore": 2}
_NONE = (1 << 64) - 1

_last: dict = {}


def mode_of(errors) -> int:
    """0, 1 or 2 for "strict", "replace", "ignore"; anything else is a ValueError (raised before
    the device is touched)."""
    if not isinstance(errors, str) or errors not in _MODES:
        raise ValueError(f"errors must be 'strict', 'replace' or 'ignore', not {errors!r}")
    return _MODES[errors]


def stats_dict(st) -> dict:
    return {"n_units": int(st.n_units), "n_bytes": int(st.n_bytes),
            "first": None if st.first == _NONE else int(st.first)}


def note(errors: str, n_units: int, n_bytes: int, first):
    """Record a non-strict call's report; first: (path or None, position) or None."""
    global _last
    _last = {"errors": errors, "n_units": int(n_units), "n_bytes": int(n_bytes), "first": first}


def last_utf8_errors() -> dict:
    """What the last call with errors="replace" or "ignore" repaired: {"errors", "n_units" (spans
    replaced or dropped), "n_bytes" (the input bytes they covered), "first": (path or None,
    position of the first span in that input) or None}.  Empty before the first such call."""
    return dict(_last)


def repair_geometry():
    """(unit, tile): the repair kernel's vector width and tile size in bytes."""
    u, t = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _lib.check(_lib.lib().bpe_utf8_repair_geometry(ctypes.byref(u), ctypes.byref(t)), "repair geometry")
    return u.value, t.value


def repair_device(t, mode: int):
    """The repaired copy of the contiguous uint8 cuda tensor t (not modified) and the stats."""
    import torch
    L = _lib.lib()
    st = _lib.Utf8Stats()
    n_out = ctypes.c_size_t(0)
    with torch.cuda.device(t.device):
        torch.cuda.current_stream().synchronize()
        src = ctypes.c_void_p(t.data_ptr()) if t.numel() else None
        _lib.check(L.bpe_utf8_repair_device(src, t.numel(), mode, None, 0, ctypes.byref(n_out), ctypes.byref(st),
                                            None), "repair_utf8")
        out = torch.empty(n_out.value, dtype=torch.uint8, device=t.device)
        if n_out.value:
            _lib.check(L.bpe_utf8_repair_device(src, t.numel(), mode, ctypes.c_void_p(out.data_ptr()), n_out.value,
                                                ctypes.byref(n_out), ctypes.byref(st), None), "repair_utf8")
    return out, stats_dict(st)


def repair_utf8(data, errors: str = "replace"):
    """data.decode("utf-8", errors).encode("utf-8") on the GPU, for errors "replace" or "ignore".

    bytes in: (bytes, stats).  A contiguous uint8 cuda tensor in: (a new tensor, stats); the input
    is not modified.  stats: {"n_units", "n_bytes", "first"} as last_utf8_errors() reports them
    (first: a position, or None)."""
    mode = mode_of(errors)
    if mode == 0:
        raise ValueError("repair_utf8 needs errors='replace' or 'ignore'")
    if isinstance(data, (bytes, bytearray, memoryview)):
        import torch
        _lib.require_device()
        raw = bytes(data)
        t = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to("cuda") if raw else \
            torch.empty(0, dtype=torch.uint8, device="cuda")
        out, st = repair_device(t, mode)
        res = out.cpu().numpy().tobytes()
    else:
        import torch
        if not (isinstance(data, torch.Tensor) and data.dtype == torch.uint8 and data.is_cuda
                and data.dim() == 1 and data.is_contiguous()):
            raise ValueError("repair_utf8 needs bytes or a contiguous 1-D uint8 cuda tensor")
        res, st = repair_device(data, mode)
    note(errors, st["n_units"], st["n_bytes"], (None, st["first"]) if st["first"] is not None else None)
    return res, st
