"""Device time of ``mpo_gp_append`` (n -> n + 1 at fixed theta) against ``mpo_gp_prepare``
of the same n + 1 points: HIP-event milliseconds, median / min / max of ``--reps`` calls
after ``--warmup``, the two interleaved call by call.

    python scripts/append_probe.py [--sizes 256,1024,2047] [--d 5] [--reps 50] [--warmup 5]
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpi_opt_amd import _lib  # noqa: E402
from mpi_opt_amd.gp import DeviceGP  # noqa: E402
from oracle import gp_ei as O  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024,2047")
    ap.add_argument("--d", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    L = _lib.lib()
    d = a.d
    amp, ls, noise = 2.0, np.linspace(0.5, 2.0, d), 0.05
    for n in (int(v) for v in a.sizes.split(",")):
        X, y = O.synthetic_problem(n + 1, d, seed=n + d)
        base = DeviceGP(X[:n], y[:n], amp, ls, noise)
        g = base.appended(X[n], y)                  # holds X, y_norm of the n + 1 points on the device
        wsb = L.mpo_gp_prepare_ws_bytes(n + 1, d)
        ws = torch.empty(wsb, dtype=torch.uint8, device=g.device)
        model = _lib.MpoGpModel()
        s = _lib.stream_handle(g.device)

        def append():
            _lib.check(L.mpo_gp_append(ctypes.byref(base.model), _lib.ptr(g._X), _lib.ptr(g._y), _lib.ptr(g._ls), noise,
                                       g.y_mean, g.y_std, ctypes.byref(model), _lib.ptr(ws), wsb, s), "mpo_gp_append")

        def prepare():
            _lib.check(L.mpo_gp_prepare(_lib.ptr(g._X), _lib.ptr(g._y), n + 1, d, _lib.ptr(g._ls), amp, noise,
                                        g.y_mean, g.y_std, ctypes.byref(model), _lib.ptr(ws), wsb, s), "mpo_gp_prepare")

        ms = {"append": [], "prepare": []}
        for it in range(a.warmup + a.reps):
            for name, fn in (("append", append), ("prepare", prepare)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if it >= a.warmup:
                    ms[name].append(e0.elapsed_time(e1))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        print(f"n {n} -> {n + 1}, d {d}: " + ", ".join(
            f"{k} median {med[k]:.3f} ms (min {min(v):.3f}, max {max(v):.3f})" for k, v in ms.items())
            + f"; prepare / append = {med['prepare'] / med['append']:.1f}x", flush=True)


if __name__ == "__main__":
    main()
