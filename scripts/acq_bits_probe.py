"""The polish objectives at fixed points of fixed models: raw results saved per library
(MPO_LIB_AB) to check that a kernel change is bit-identical, and the wall time of one
polish-sized round (15 points, 1 thread).  Recorded: ``acq_grad`` (16-wave form up to
n = 700, 4-wave form at n = 915), ``acq_grad_ps`` f, g and parts at n = 96 and 915,
``DevicePaths.grad`` at (n, d, F, s) = (57, 3, 64, 4), and x, f, stats of ``polish``,
``polish_ps`` and ``DevicePaths.polish`` from fixed starts at n = 96.
Usage: acq_bits_probe.py OUT.npz [REF.npz]"""
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import scripts.ab_lib  # noqa: E402,F401
from mpi_opt_amd import _lib  # noqa: E402
from mpi_opt_amd import gp as G  # noqa: E402
from mpi_opt_amd.gp_fit import FMIN_FTOL  # noqa: E402
from mpi_opt_amd.paths import draw_paths  # noqa: E402
from oracle import gp_ei as O  # noqa: E402

DEV = "cuda:0"


def model(n, d):
    X, y = O.synthetic_problem(n, d, seed=n)
    rs = np.random.RandomState(d)
    gp = G.DeviceGP(X, y, amp=1.3, length_scale=rs.uniform(0.2, 1.5, d), noise=1e-4, device=DEV)
    return X, y, rs, gp


def time_model(X, y, d):
    """The log-time model of the cost-aware objective over the same observations."""
    rs = np.random.RandomState(1000 + d)
    t = np.log(0.5 + np.abs(y - np.min(y)) + rs.rand(len(y)))
    return G.DeviceGP(X, t, amp=0.8, length_scale=rs.uniform(0.3, 1.2, d), noise=1e-3, device=DEV)


def record(out, name, res, pairs=None):
    """x, f, stats | rounds of one polish; ``pairs``: the public wrapper's [(x, f)] of the same runs."""
    x, f, stats, rounds = res
    out[name + "_x"], out[name + "_f"], out[name + "_stats"] = x, f, np.append(stats.reshape(-1), rounds)
    if pairs is not None:
        assert all(p[0].tobytes() == x[r].tobytes() and p[1] == f[r] for r, p in enumerate(pairs)), name
    print(f"{name}: {rounds} rounds, nfev {stats[:, 1].tolist()}", flush=True)


def main():
    out = {}
    for n, d in [(57, 3), (96, 5), (256, 5), (448, 10), (700, 6), (915, 6)]:
        X, y, rs, gp = model(n, d)
        P = rs.rand(15, d)
        codes = np.array([_lib.MPO_ACQ_EI, _lib.MPO_ACQ_PI, _lib.MPO_ACQ_LCB] * 5, dtype=np.int32)
        y_opt = float(np.min(y))
        f, g = gp.acq_grad(P, codes, y_opt)
        out[f"n{n}_f"], out[f"n{n}_g"] = f, g
        for _ in range(20):
            gp.acq_grad(P, codes, y_opt)
        R = 300
        t0 = time.perf_counter()
        for _ in range(R):
            gp.acq_grad(P, codes, y_opt)
        print(f"n={n} [{gp.acq_grad_path} waves]: {(time.perf_counter() - t0) / R * 1e6:.1f} us per 15-point round",
              flush=True)
        if n in (96, 915):
            tg = time_model(X, y, d)
            pc = np.array([_lib.MPO_ACQ_EI, _lib.MPO_ACQ_PI] * 8, dtype=np.int32)[:15]
            for k, v in zip("fgp", G.acq_grad_ps(gp, tg, P, pc, y_opt, want_parts=True)):
                out[f"ps{n}_{k}"] = v
        if n == 96:
            bounds = np.array([[0.0, 1.0]] * d)
            # the wrappers' own runner, for the stats that polish / polish_ps do not return
            ref_m, ref_t = ctypes.byref(gp.model), ctypes.byref(tg.model)
            tail = (FMIN_FTOL, 20, 1e-5, 15000, gp._ensure_ag(15), gp._ag_stream)
            record(out, "polish", G._run_polish("mpo_gp_polish_host", (ref_m,), (y_opt, 0.01, 1.96), P, codes,
                                                bounds, *tail), gp.polish(P, codes, y_opt, 0.01, 1.96, bounds, FMIN_FTOL))
            record(out, "polish_ps", G._run_polish("mpo_gp_polish_ps_host", (ref_m, ref_t), (y_opt, 0.01), P, pc,
                                                   bounds, *tail), G.polish_ps(gp, tg, P, pc, y_opt, 0.01, bounds, FMIN_FTOL))
            dp = gp.paths(*draw_paths(np.random.RandomState(7), 64, d, 4, n))
            record(out, "paths_polish", dp.polish(P[:8], np.arange(8) % 4, bounds))
        if n == 57:
            dp = gp.paths(*draw_paths(np.random.RandomState(7), 64, d, 4, n))
            f, g = dp.grad(P, np.arange(15) % 4)
            out["paths_grad_f"], out["paths_grad_g"] = f.cpu().numpy(), g.cpu().numpy()
    np.savez(sys.argv[1], **out)
    if len(sys.argv) > 2:
        ref = np.load(sys.argv[2])
        same = {k: ref[k].tobytes() == out[k].tobytes() for k in out}
        print("differing:", [k for k, v in same.items() if not v])
        print(f"bit-identical: {len(ref.files) == len(out) and all(same.values())} ({len(out)} arrays)")


if __name__ == "__main__":
    main()
