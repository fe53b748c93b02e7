"""The joint-posterior kernels at their size limits (n = 2048, m = 4096) against a torch fp64
restatement on the device: prints the covariance, mean, sd and sample differences and how
many argmins agree.  Far past what the 80-bit reference of tests/test_gp_joint_gpu.py can
build in seconds; a figure, not a test.

    python scripts/joint_limits_check.py
"""
import os
import sys

import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpi_opt_amd.gp import DeviceGP
from oracle import gp_ei as O

def matern(A, B, amp):
    # row chunks: the direct-difference cdist launches one workgroup per pair
    r = torch.cat([torch.cdist(A[i:i + 512], B, compute_mode="donot_use_mm_for_euclid_dist")
                   for i in range(0, A.shape[0], 512)])
    k = r * 5 ** 0.5
    return amp * (1 + k + k * k / 3) * torch.exp(-k)

for n, m, s, d in ((2048, 4096, 64, 5), (1300, 4095, 33, 32), (2047, 1000, 300, 10)):
    amp, ls, noise = 2.0, np.linspace(0.5, 2.0, d), 0.05
    X, y = O.synthetic_problem(n, d, seed=n + d)
    g = DeviceGP(X, y, amp, ls, noise)
    C = O.synthetic_candidates(m, d, seed=7)
    Z = np.random.RandomState(3).standard_normal((m, s))
    mu, cov = g.posterior_cov(C)
    out = g.sample(C, Z, jitter=1e-8)
    lst = torch.from_numpy(ls).cuda()
    Ct, Xt = torch.from_numpy(C).cuda() / lst, torch.from_numpy(X).cuda() / lst
    W = g.L_inverse()
    Ks = matern(Ct, Xt, amp)
    V = Ks @ W.T
    Sn = matern(Ct, Ct, amp) - V @ V.T
    mu_r = g.y_mean + g.y_std * (Ks @ g.alpha())
    e_cov = float((cov - g.y_std ** 2 * Sn).abs().max()) / (amp * g.y_std ** 2)
    e_mu = float((mu - mu_r).abs().max())
    Lc = torch.linalg.cholesky(Sn + 1e-8 * amp * torch.eye(m, dtype=torch.float64, device="cuda"))
    S = mu_r[None, :] + g.y_std * (Lc @ torch.from_numpy(Z).cuda()).T
    e_s = float((out["samples"] - S).abs().max()) / (g.y_std * amp ** 0.5)
    same = bool(torch.equal(out["argmin"], out["samples"].argmin(1)))
    agree = int((out["argmin"] == S.argmin(1)).sum())
    sd = g.score(C, float(np.min(y)), acqs=("EI",))["sd"]
    e_sd = float(((cov.diagonal().clamp_min(0).sqrt() - sd).abs() / sd).max())
    print(f"n={n} m={m} s={s} d={d} path={g.score_path}: info {out['info']}, cov err {e_cov:.3e} of amp y_std^2, "
          f"mu err {e_mu:.3e}, sqrt(diag) vs sd {e_sd:.3e}, samples err {e_s:.3e} of scale, symmetric "
          f"{bool(torch.equal(cov, cov.T))}, argmin == argmin(own samples) {same}, == torch's {agree}/{s}", flush=True)
