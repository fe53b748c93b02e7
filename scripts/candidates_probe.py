"""The pieces of one proposal with host-drawn and with device-drawn candidates
(``Optimizer(candidates=...)``): sample, host-to-device copy, score (top-k of the three
acquisitions), gather + polish, total -- host-clock milliseconds, each piece ended by a
device synchronise, median and range over ``--reps`` proposals after ``--warmup``.  The
two sources alternate proposal by proposal in one process, on one fixed-theta model of
``--told`` points.  Also the sampler's device time (HIP events) beside a
``torch.Tensor.fill_`` of the same tensor, the practical store yardstick.

    python scripts/candidates_probe.py [--space mnist,real10] [--n-points 1000000] [--told 200]
                                       [--source both|host|device] [--reps 20] [--warmup 3]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpi_opt_amd.blocks import _device_topk  # noqa: E402
from mpi_opt_amd.candidates import sample_transformed  # noqa: E402
from mpi_opt_amd.models import mnist_space  # noqa: E402
from mpi_opt_amd.optimizer import DRIVER, GPModel, polish_lockstep  # noqa: E402
from mpi_opt_amd.space import Real, Space  # noqa: E402

ACQS = ("EI", "LCB", "PI")
PIECES = ("sample", "copy", "score", "polish", "total")


def proposal(source, space, est, n_points, rng, dev):
    """One proposal's pieces in seconds; the candidates end up on the device either way."""
    y_opt = float(np.min(est.y))
    t0 = time.perf_counter()
    if source == "device":
        X = sample_transformed(space, n_points, int(rng.randint(0, np.iinfo(np.int32).max)), dev)
        torch.cuda.synchronize(dev)
        t1 = t2 = time.perf_counter()
    else:
        Xh = space.rvs_transformed(n_samples=n_points, random_state=rng)
        t1 = time.perf_counter()
        X = torch.from_numpy(Xh).to(dev)
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
    top = _device_topk(est, X, y_opt, ACQS, 0.01, 1.96, 5)       # ends in the copy of the winners' indices
    t3 = time.perf_counter()
    idx = np.concatenate([top[a][1] for a in ACQS])
    starts = X[torch.from_numpy(idx).to(dev)].cpu().numpy()      # the 15 winning rows
    polish_lockstep(est, list(starts), [a for a in ACQS for _ in range(5)], y_opt, 0.01, 1.96,
                    space.transformed_bounds, driver=DRIVER)
    t4 = time.perf_counter()
    return dict(zip(PIECES, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t4 - t0)))


def event_ms(fn, reps):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--space", default="mnist", help="mnist (option3: 4 Integer + 1 Real), real10, or both: mnist,real10")
    ap.add_argument("--n-points", type=int, default=1_000_000, dest="n_points")
    ap.add_argument("--told", type=int, default=200)
    ap.add_argument("--source", default="both", choices=["both", "host", "device"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    for name in a.space.split(","):
        if name not in ("mnist", "real10"):
            ap.error(f"--space {name!r}: mnist or real10")
        probe(a, name)


def probe(a, space_name):
    dev = torch.device("cuda:0")
    space = Space(mnist_space() if space_name == "mnist" else [Real(0.0, 1.0) for _ in range(10)])
    d = space.transformed_n_dims
    rng = np.random.RandomState(1)
    Xt = space.rvs_transformed(a.told, rng)
    y = np.sum((Xt - 0.4) ** 2, axis=1) + 0.05 * rng.randn(a.told)
    est = GPModel(Xt, y, 1.5, np.linspace(0.4, 1.3, d), 0.02, device=dev)
    est.dev
    sources = ("host", "device") if a.source == "both" else (a.source,)
    ms = {s: {p: [] for p in PIECES} for s in sources}
    for it in range(a.warmup + a.reps):
        for s in sources:
            t = proposal(s, space, est, a.n_points, rng, dev)
            if it >= a.warmup:
                for p in PIECES:
                    ms[s][p].append(1e3 * t[p])
    print(f"space {space_name} (d = {d}), n_points {a.n_points}, told {a.told}, {a.reps} proposals per source "
          f"after {a.warmup} warm-up, alternating; host-clock ms: median (min .. max)", flush=True)
    for s in sources:
        print(f"  {s:6s} " + "  ".join(f"{p} {np.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"
                                       for p, v in ms[s].items()), flush=True)
    if len(sources) == 2:
        h, g = np.median(ms["host"]["total"]), np.median(ms["device"]["total"])
        print(f"  total host / device = {h / g:.1f}x", flush=True)
    # the sampler alone, HIP events, beside a fill_ of the same tensor
    out = torch.empty((a.n_points, d), dtype=torch.float64, device=dev)
    event_ms(lambda: out.fill_(0.5), a.warmup)
    event_ms(lambda: sample_transformed(space, a.n_points, 7, dev), a.warmup)
    fill, samp = [], []
    for _ in range(a.reps):
        fill += event_ms(lambda: out.fill_(0.5), 1)
        samp += event_ms(lambda: sample_transformed(space, a.n_points, 7, dev), 1)
    gb = out.numel() * 8 / 1e9
    for name, v in (("mpo_space_sample", samp), ("fill_", fill)):
        print(f"  {name}: {np.median(v):.4f} ms ({min(v):.4f} .. {max(v):.4f}) device events, "
              f"{gb / (np.median(v) * 1e-3):.0f} GB/s written ({gb * 1e3:.1f} MB)", flush=True)


if __name__ == "__main__":
    main()
