"""Thompson ask batches against the constant-liar ones, and the device time of the joint
posterior they draw from.

    python scripts/thompson_probe.py batches [--ask-n 256] [--rounds 9]
    python scripts/thompson_probe.py kernels [--sizes 256:2048:256,2048:4096:256] [--reps 50] [--warmup 5]

``batches``: a lone ``ask(N)`` after 256 tells (bench.py's ask256 leg, the setup of
scripts/ask_chain_probe.py), three arms interleaved in rounds in one process -- ``cl_min``
with ``lie_refit="every"`` (skopt), ``cl_min`` with ``lie_refit="never"`` and ``thompson``
-- median and min-max of the seconds per batch, and the host-clock split of the Thompson
step (each part ends in a device synchronise).

``kernels``: HIP-event milliseconds of the stages of ``mpo_gp_sample`` at (n, m, s), median
of ``--reps`` after ``--warmup``.  The C ABI launches whole sequences, so the stages are
timed as nested calls and reported as differences of medians:
    V + cov        mpo_gp_posterior_cov
    + factor       mpo_gp_sample with samples = argmin = NULL (V, cov, blocked Cholesky)
    + sample       mpo_gp_sample with every output
Per-kernel times proper come from ``rocprofv3 --kernel-trace --stats -- python
scripts/thompson_probe.py kernels`` in a run of its own.
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


def told_optimizer(**kw):
    from mpi_opt_amd.models import mnist_space

    rng = np.random.RandomState(256)
    opt = OPT.Optimizer(mnist_space(), random_state=13579, device="cuda:0", **kw)
    pts = opt.space.rvs(n_samples=256, random_state=rng)
    ys = [float(((p[0] - 30) / 40) ** 2 + ((p[3] - 120) / 150) ** 2 + (p[4] - 0.3) ** 2 + 0.1 * rng.rand())
          for p in pts]
    opt.tell(pts[:-1], ys[:-1], fit=False)
    opt.tell(pts[-1], ys[-1])
    return opt


def stats(v):
    return f"median {np.median(v):.4f} (min {min(v):.4f}, max {max(v):.4f})"


def batches(a):
    import torch

    arms = {"cl_min every": ({}, "cl_min"), "cl_min never": ({"lie_refit": "never"}, "cl_min"),
            "thompson": ({}, "thompson")}
    secs = {k: [] for k in arms}
    split = {"copy_and_fit_s": [], "candidates_s": [], "sample_s": [], "dedupe_s": []}
    step = OPT._thompson_step
    step_start = []

    def timed_step(opt, r):
        torch.cuda.synchronize()
        step_start.append(time.perf_counter())
        out = step(opt, r)
        for k, v in opt.thompson_times.items():
            split[k].append(v)
        return out

    OPT._thompson_step = timed_step
    for rnd in range(a.rounds + 1):                # round 0 warms every arm up and is dropped
        for name, (kw, strategy) in arms.items():
            opt = told_optimizer(**kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            X = opt.ask(a.ask_n, strategy)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if name == "thompson":                 # the copy, its one fit and its own proposal
                split["copy_and_fit_s"].append(step_start[-1] - t0)
            if rnd:
                secs[name].append(dt)
            print(f"round {rnd} {name}: ask({a.ask_n}) {dt:.4f} s, first point {list(X[0])}", flush=True)
    for name, v in secs.items():
        print(f"{name}: {len(v)} batches, seconds {stats(v)}")
    print("thompson split (seconds, host clock, warm-up round dropped):")
    for k, v in split.items():
        print(f"  {k}: {stats(v[1:])}")


def kernels(a):
    import torch

    from mpi_opt_amd.gp import DeviceGP
    from oracle import gp_ei as O

    L = _lib.lib()
    d = a.d
    amp, ls, noise = 2.0, np.linspace(0.5, 2.0, d), 0.05
    for n, m, s in (tuple(int(v) for v in sz.split(":")) for sz in a.sizes.split(",")):
        X, y = O.synthetic_problem(n, d, seed=n + d)
        g = DeviceGP(X, y, amp, ls, noise)
        dev = g.device
        C = g.as_candidates(O.synthetic_candidates(m, d, seed=7))
        Z = torch.from_numpy(np.random.RandomState(3).standard_normal((m, s))).to(dev)
        ws, wsb = g._ensure_joint_ws(m, s)
        mu = torch.empty(m, dtype=torch.float64, device=dev)
        cov = torch.empty(m, m, dtype=torch.float64, device=dev)
        samples = torch.empty(s, m, dtype=torch.float64, device=dev)
        argmin = torch.empty(s, dtype=torch.int64, device=dev)
        info = torch.empty(1, dtype=torch.int32, device=dev)
        st = _lib.stream_handle(dev)
        P, md = _lib.ptr, ctypes.byref(g.model)

        def v_cov():
            _lib.check(L.mpo_gp_posterior_cov(md, P(C), m, P(mu), P(cov), m, P(ws), wsb, st), "mpo_gp_posterior_cov")

        def factor():
            _lib.check(L.mpo_gp_sample(md, P(C), m, P(Z), s, a.jitter, None, None, P(info), P(ws), wsb, st),
                       "mpo_gp_sample")

        def full():
            _lib.check(L.mpo_gp_sample(md, P(C), m, P(Z), s, a.jitter, P(samples), P(argmin), P(info), P(ws), wsb,
                                       st), "mpo_gp_sample")

        ms = {"v_cov": [], "factor": [], "full": []}
        for it in range(a.warmup + a.reps):
            for name, fn in (("v_cov", v_cov), ("factor", factor), ("full", full)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if it >= a.warmup:
                    ms[name].append(e0.elapsed_time(e1))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        print(f"n {n} m {m} s {s} d {d}, ws {wsb / 2**20:.1f} MiB, info {int(info.item())}: " + ", ".join(
            f"{k} {stats(v)} ms" for k, v in ms.items()) +
            f"; V + cov {med['v_cov']:.3f}, factor {med['factor'] - med['v_cov']:.3f}, "
            f"sample + argmin {med['full'] - med['factor']:.3f} ms", flush=True)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    b = sub.add_parser("batches")
    b.add_argument("--ask-n", type=int, default=256)
    b.add_argument("--rounds", type=int, default=9)
    k = sub.add_parser("kernels")
    k.add_argument("--sizes", default="256:2048:256,2048:4096:256")
    k.add_argument("--d", type=int, default=5)
    k.add_argument("--reps", type=int, default=50)
    k.add_argument("--warmup", type=int, default=5)
    k.add_argument("--jitter", type=float, default=1e-8)
    a = ap.parse_args()
    (batches if a.mode == "batches" else kernels)(a)


if __name__ == "__main__":
    main()
