"""The shapes at which the refit objective (``csrc/gp_fit.hip``: LML and gradient)
changes kernel, template instantiation or launch sequence, and a plain-Python
restatement of the rule that picks them.  No GPU import: the host test
(``test_lml_cases_host.py``) guards the table's coverage, the GPU test
(``test_gp_fit_shapes_gpu.py``) runs it.

The rule (``fit_dp``, ``sw_np``, ``use_split``, ``fit_fused_split`` and
``launch_split_group``'s ``fuse_build`` in gp_fit.hip):

* ``dp = fit_dp(d)``: the padded dimension, one template instantiation each;
* the single-workgroup "panel" Cholesky kernel for n <= 48, the multi-workgroup
  "split" block sweep past it; ``MPO_FIT_KERNEL=panel`` keeps the panel kernel up
  to the LDS limit n = 200, ``MPO_FIT_KERNEL=split`` takes the sweep from n = 17;
* the sweep is "fused" (K build and finish in one launch each, pinned in-place I/O
  on the host-staged entry) while ``sw_np(n) * dp <= 8192``, and runs the separate
  ``sw_xs`` / ``sw_build`` / ``sw_pairs`` / ``sw_final`` kernels past that.
"""
import functools
from collections import namedtuple

import numpy as np

K_SW_NB = 32          # kSwNb: the sweep's pivot-block width
K_SPLIT_MIN_N = 48    # kSplitMinN: the last n of the panel kernel
K_FIT_LDS_MAX_N = 200  # kFitLdsMaxN: the panel kernel's packed factor fills the LDS
K_MAX_OBS = 2048      # mpo::kMaxObs
K_FUSED_DOUBLES = 8192  # 64 KiB of divided X rows: np * dp past it is unfused
K_MAX_GROUP = 40      # kMaxGroup: thetas per launch set of the sweep
DPS = (4, 8, 12, 16, 32)


def fit_dp(d):
    for dp in DPS:
        if d <= dp:
            return dp
    return -1


def sw_np(n):
    return (n + K_SW_NB - 1) // K_SW_NB * K_SW_NB


def use_split(n, forced=None):
    if forced == "split":
        return 16 < n <= K_MAX_OBS
    if forced == "panel" and n <= K_FIT_LDS_MAX_N:
        return False
    return n > K_SPLIT_MIN_N


def path(n, d, forced=None):
    """(kernel, dp, fused) of one evaluation: kernel is 'panel', 'split-fused' or
    'split-unfused'; fused is None on the panel kernel."""
    dp = fit_dp(d)
    if dp < 0 or not 0 < n <= K_MAX_OBS:
        raise ValueError(f"n={n} d={d} outside n <= {K_MAX_OBS}, d <= 32")
    if not use_split(n, forced):
        return "panel", dp, None
    fused = sw_np(n) * dp <= K_FUSED_DOUBLES
    return ("split-fused" if fused else "split-unfused"), dp, fused


#: every (kernel, dp) that exists: sw_np(2048) * 4 = 8192 keeps dp = 4 fused at every n
COMBINATIONS = ([("panel", dp) for dp in DPS] + [("split-fused", dp) for dp in DPS]
                + [("split-unfused", dp) for dp in DPS if dp > 4])

Case = namedtuple("Case", "n d forced")

# each shape is the smallest that reaches its edge
PANEL = [Case(n, d, None) for n, d in
         # n = 1, 2; the panel width 8 (7, 8, 9); two panels; no padding at d = dp (4, 8, 12,
         # 16, 32); the 32-wide edge; the last n before the split
         [(1, 1), (2, 1), (7, 4), (8, 8), (9, 12), (16, 16), (17, 13), (33, 32), (48, 32)]]
PANEL_FORCED = [Case(200, 17, "panel")]          # dp = 32 at the LDS limit
SPLIT_FUSED = [Case(n, d, None) for n, d in
               # the first n past the switch; np a multiple of 32 and not; the fused limits
               # 256 x 32, 512 x 16, 2048 x 4 (the ABI's largest n)
               [(49, 16), (65, 17), (96, 32), (256, 32), (512, 16), (2048, 4)]]
# the last fused n of dp = 12 and 8, next to the first unfused ones below: the two
# instantiations of the fused sweep that the shapes above leave out
SPLIT_FUSED_LIMITS = [Case(672, 12, None), Case(1024, 8, None)]
SPLIT_FORCED = [Case(17, 32, "split")]           # one pivot block, identity padding, dp = 32
SPLIT_UNFUSED = [Case(n, d, None) for n, d in
                 # the smallest n per dp (32, 16, 12, 8) past the fused limit
                 [(257, 17), (513, 13), (673, 9), (1025, 5)]]
CASES = PANEL + PANEL_FORCED + SPLIT_FUSED + SPLIT_FUSED_LIMITS + SPLIT_FORCED + SPLIT_UNFUSED

NOISES = (1e-2, 0.2)


def case_id(c):
    return f"n{c.n}_d{c.d}" + (f"_{c.forced}" if c.forced else "")


def problem(n, d):
    """(X, y, y normalised as sklearn's normalize_y and the oracle do): the oracle takes
    the raw y, the device and the longdouble reference the normalised one."""
    from oracle import gp_ei as O

    X, y = O.synthetic_problem(n, d, seed=n + d)
    s = float(np.std(y))
    return X, y, (y - np.mean(y)) / (s if s != 0.0 else 1.0)


def thetas(n, d):
    """Two thetas per case from one generator: amp in [0.5, 3), length scales in
    [0.3, 3), noise 1e-2 and 0.2."""
    r = np.random.RandomState(n)
    return np.array([np.log(np.r_[r.uniform(0.5, 3), r.uniform(0.3, 3, d), noise]) for noise in NOISES])


def gram(X, theta):
    """K as the oracle and the device build it: amp * Matern52 + (noise + 1e-10) I."""
    from oracle import gp_ei as O

    n, d = X.shape
    amp, ls, noise = np.exp(theta[0]), np.exp(theta[1:d + 1]), np.exp(theta[d + 1])
    M = O.matern52(X, X, ls, 1.0)
    np.fill_diagonal(M, 1.0)
    return amp * M + (noise + O.SKOPT_ALPHA_JITTER) * np.eye(n)


def lml_longdouble(K, yn):
    """The LML of K in 80-bit arithmetic: a left-looking Cholesky by columns, the
    forward solve, -z.z / 2 - sum log L_jj - n / 2 log 2 pi."""
    ld = np.longdouble
    A = np.asarray(K, dtype=ld)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=ld)
    for j in range(n):
        c = A[j:, j] - L[j:, :j] @ L[j, :j]
        L[j, j] = np.sqrt(c[0])
        L[j + 1:, j] = c[1:] / L[j, j]
    y = np.asarray(yn, dtype=ld)
    z = np.zeros(n, dtype=ld)
    for i in range(n):
        z[i] = (y[i] - L[i, :i] @ z[:i]) / L[i, i]
    two_pi = ld("6.283185307179586476925286766559005768")
    return -(z @ z) / 2 - np.log(np.diag(L)).sum() - ld(n) / 2 * np.log(two_pi)


@functools.lru_cache(maxsize=None)
def reference(n, d):
    """The case's inputs and the fp64 oracle's answers, computed once per process and
    shared (treat the arrays as read-only): X, yn, thetas [2, d + 2], lml [2],
    grad [2, d + 2]."""
    from oracle import gp_ei as O

    X, y, yn = problem(n, d)
    T = thetas(n, d)
    out = [O.lml_and_grad(X, y, t) for t in T]
    ref = (X, yn, T, np.array([o[0] for o in out]), np.stack([o[1] for o in out]))
    for a in ref:
        a.setflags(write=False)
    return ref
