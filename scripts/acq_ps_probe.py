"""What the cost-aware acquisitions EIps / PIps cost on the device.

    python scripts/acq_ps_probe.py kernels [--reps 20] [--warmup 3]
    python scripts/acq_ps_probe.py proposal [--rounds 7]

``kernels``: HIP-event milliseconds, median of ``--reps`` after ``--warmup``.
``mpo_gp_acq_ps_score`` (EI, values and top-5) at (n, d, m) = (200, 10, 1e4) and (200, 10, 1e6),
interleaved with the two plain ``mpo_gp_acq_score`` calls it contains on the same models (EI
rows only; mu / sd only): the ps call's time over the sum of the two is what the finish pass and
the merge add.  Then ``mpo_gp_acq_ps_grad`` at (n, batch) = (256, 5) against ``mpo_gp_acq_grad``.

``proposal``: one ``tell`` at n = 64, d = 5 with 10 000 candidates, ``acq_func="EI"`` against
``"EIps"``, the arms interleaved in one process, ``--rounds`` each after a warm-up round: seconds
per tell and the split into fit, prepare, score and polish (``optimizer.STATS``).  The EIps fit is
two fits.
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpi_opt_amd import _lib  # noqa: E402
from mpi_opt_amd import optimizer as OPT  # noqa: E402


def med(v):
    return float(np.median(v))


def event_ms(fn, reps, warmup):
    import torch

    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def pair(n, d, seed=0):
    from mpi_opt_amd.gp import DeviceGP
    from oracle.gp_ei import synthetic_problem

    X, y = synthetic_problem(n, d, seed=seed)
    rng = np.random.RandomState(seed + 1)
    logt = 1.2 * np.sin(X @ rng.randn(d)) + 0.8 * X[:, 0] + 0.05 * rng.randn(n)
    ls_f, ls_t = 0.45 + 0.11 * (np.arange(d) % 5), 0.95 - 0.07 * (np.arange(d) % 4)
    return (DeviceGP(X, y, 1.3, ls_f, 0.02, device="cuda:0"), DeviceGP(X, logt, 0.8, ls_t, 0.05, device="cuda:0"),
            float(np.min(y)))


def kernels(a):
    import torch

    L = _lib.lib()
    ref = ctypes.byref
    s = _lib.stream_handle()
    fg, tg, y_opt = pair(200, 10)
    for m in (10_000, 1_000_000):
        c = torch.rand(m, 10, dtype=torch.float64, device="cuda:0")
        need = L.mpo_gp_acq_ps_ws_bytes(ref(fg.model), ref(tg.model), m, 5)
        ws = torch.empty(need, dtype=torch.uint8, device="cuda:0")
        wsp = torch.empty(L.mpo_gp_score_ws_bytes(ref(fg.model), m, 0), dtype=torch.uint8, device="cuda:0")
        vals = torch.empty(3, m, dtype=torch.float64, device="cuda:0")
        mu, sd = torch.empty(m, dtype=torch.float64, device="cuda:0"), torch.empty(m, dtype=torch.float64, device="cuda:0")
        tki, tkv = torch.empty(2, 5, dtype=torch.int64, device="cuda:0"), torch.empty(2, 5, dtype=torch.float64, device="cuda:0")

        def ps():
            _lib.check(L.mpo_gp_acq_ps_score(ref(fg.model), ref(tg.model), c.data_ptr(), m, y_opt, 0.01, 1,
                                             vals.data_ptr(), None, 5, tki.data_ptr(), tkv.data_ptr(), ws.data_ptr(),
                                             need, s))

        def plain_f():
            _lib.check(L.mpo_gp_acq_score(ref(fg.model), c.data_ptr(), m, y_opt, 0.01, 0.0, 1, None, None,
                                          vals.data_ptr(), 0, None, None, wsp.data_ptr(), wsp.numel(), s))

        def plain_t():
            _lib.check(L.mpo_gp_acq_score(ref(tg.model), c.data_ptr(), m, 0.0, 0.0, 0.0, 1, mu.data_ptr(), sd.data_ptr(),
                                          None, 0, None, None, wsp.data_ptr(), wsp.numel(), s))

        t = {"ps": [], "f": [], "t": []}
        for fn in (ps, plain_f, plain_t):
            event_ms(fn, 0, a.warmup)
        for _ in range(a.reps):                        # interleaved: one of each per round
            t["ps"] += event_ms(ps, 1, 0)
            t["f"] += event_ms(plain_f, 1, 0)
            t["t"] += event_ms(plain_t, 1, 0)
        both = med(t["f"]) + med(t["t"])
        print(f"score n=200 d=10 m={m}: ps {med(t['ps']):.4f} ms [{min(t['ps']):.4f}, {max(t['ps']):.4f}]; plain EI rows "
              f"{med(t['f']):.4f} ms + plain mu/sd {med(t['t']):.4f} ms = {both:.4f} ms; ps / sum = {med(t['ps']) / both:.4f}",
              flush=True)
    fg, tg, y_opt = pair(256, 5)
    x = torch.rand(5, 5, dtype=torch.float64, device="cuda:0")
    acq = torch.ones(5, dtype=torch.int32, device="cuda:0")
    f, g = torch.empty(5, dtype=torch.float64, device="cuda:0"), torch.empty(5, 5, dtype=torch.float64, device="cuda:0")
    t = {"ps": [], "plain": []}

    def ps_grad():
        _lib.check(L.mpo_gp_acq_ps_grad(ref(fg.model), ref(tg.model), x.data_ptr(), 5, acq.data_ptr(), y_opt, 0.01,
                                        f.data_ptr(), g.data_ptr(), None, s))

    def plain_grad():
        _lib.check(L.mpo_gp_acq_grad(ref(fg.model), x.data_ptr(), 5, acq.data_ptr(), y_opt, 0.01, 1.96, f.data_ptr(),
                                     g.data_ptr(), s))

    for fn in (ps_grad, plain_grad):
        event_ms(fn, 0, a.warmup)
    for _ in range(a.reps):
        t["ps"] += event_ms(ps_grad, 1, 0)
        t["plain"] += event_ms(plain_grad, 1, 0)
    print(f"grad n=256 batch=5: mpo_gp_acq_ps_grad {med(t['ps']) * 1e3:.1f} us [{min(t['ps']) * 1e3:.1f}, "
          f"{max(t['ps']) * 1e3:.1f}]; mpo_gp_acq_grad {med(t['plain']) * 1e3:.1f} us [{min(t['plain']) * 1e3:.1f}, "
          f"{max(t['plain']) * 1e3:.1f}]; ratio {med(t['ps']) / med(t['plain']):.3f}", flush=True)


def proposal(a):
    import torch

    from mpi_opt_amd.models import mnist_space
    from mpi_opt_amd.optimizer import Optimizer

    rng = np.random.RandomState(3)
    sp = Optimizer(mnist_space(), random_state=0, n_initial_points=10 ** 6).space
    X = sp.rvs(64, random_state=rng)
    vals = [float(((x[0] - 30) / 40) ** 2 + ((x[3] - 120) / 150) ** 2 + (x[4] - 0.3) ** 2) for x in X]
    cost = [float(0.2 + 1e-3 * x[0] * x[2] + 1e-3 * x[3]) for x in X]
    keys = ("refit_s", "prepare_s", "score_s", "polish_s")
    secs = {"EI": [], "EIps": []}
    split = {k: {q: [] for q in keys} for k in secs}
    for rnd in range(a.rounds + 1):                    # round 0 warms both arms up and is dropped
        for arm in secs:
            opt = Optimizer(mnist_space(), acq_func=arm, random_state=1, n_initial_points=10, device="cuda:0",
                            acq_optimizer_kwargs={"n_points": 10000})
            OPT.reset_stats()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            opt.tell(X, list(zip(vals, cost)) if arm == "EIps" else vals)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rnd:
                secs[arm].append(dt)
                for q in keys:
                    split[arm][q].append(OPT.STATS[q])
    for arm in secs:
        print(f"tell n=64 d=5, 10000 candidates, {arm}: {med(secs[arm]) * 1e3:.2f} ms [{min(secs[arm]) * 1e3:.2f}, "
              f"{max(secs[arm]) * 1e3:.2f}]; " + ", ".join(f"{q[:-2]} {med(split[arm][q]) * 1e3:.2f} ms" for q in keys),
              flush=True)
    print(f"EIps / EI = {med(secs['EIps']) / med(secs['EI']):.3f}")


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=["kernels", "proposal"])
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--rounds", type=int, default=7)
    args = p.parse_args()
    {"kernels": kernels, "proposal": proposal}[args.mode](args)
