"""Inputs of the joint-posterior tests (tests/test_gp_joint_gpu.py), importable by the test
and runnable as a script in a fresh process:

    python tests/joint_cases.py OUT.npz

writes the covariance and the samples of ``PATH_CASE`` as the device computes them under
the environment of that process (``MPO_GP_SCORE=streamed`` is read at prepare time).

The inputs are those of the other GP tests: ``O.synthetic_problem(n, d, seed=n + d)``,
theta = (2.0, linspace(0.5, 2, d), 0.05), ``O.synthetic_candidates(m, d, seed=7)`` and
``Z = RandomState(3).standard_normal((m, s))``.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import gp_ei as O  # noqa: E402

AMP, NOISE = 2.0, 0.05
JITTER = 1e-10
PATH_CASE = (64, 4, 96, 32)      # (n, d, m, s) of the path- and model-independence tests


def theta(d):
    return AMP, np.linspace(0.5, 2.0, d), NOISE


def inputs(n, d, m, s=0):
    X, y = O.synthetic_problem(n, d, seed=n + d)
    C = O.synthetic_candidates(m, d, seed=7)
    Z = np.random.RandomState(3).standard_normal((m, s)) if s else None
    return X, y, C, Z


def device_gp(X, y, d):
    from mpi_opt_amd.gp import DeviceGP

    amp, ls, noise = theta(d)
    return DeviceGP(X, y, amp, ls, noise)


def device_joint(g, C, Z):
    """(mu, cov, samples, argmin, info) of the DeviceGP ``g`` as numpy arrays."""
    mu, cov = g.posterior_cov(C)
    out = g.sample(C, Z, jitter=JITTER)
    return (mu.cpu().numpy(), cov.cpu().numpy(), out["samples"].cpu().numpy(), out["argmin"].cpu().numpy(),
            out["info"])


if __name__ == "__main__":
    n, d, m, s = PATH_CASE
    X, y, C, Z = inputs(n, d, m, s)
    g = device_gp(X, y, d)
    mu, cov, samples, argmin, info = device_joint(g, C, Z)
    np.savez(sys.argv[1], mu=mu, cov=cov, samples=samples, argmin=argmin, info=info, score_path=g.score_path)
