"""The sizes, widths and inputs at which what lies between the refit and scoring changes
launch geometry, path or arithmetic regime -- ``mpo_gp_prepare``'s blocked factorisation
(``blocked_factor`` in ``csrc/gp.hip``), the polish objective ``mpo_gp_acq_grad`` and the
three exported primitives ``mpo_gp_kernel_matrix`` / ``mpo_chol_f64`` / ``mpo_trsm_f64``
-- with a plain-Python restatement of the rules that decide them.  No GPU or torch
import: the host test (``test_factor_cases_host.py``) guards the tables and the
references, the GPU test (``test_gp_factor_shapes_gpu.py``) runs them.

What decides how a model is factored (``blocked_factor``):

* the matrix is padded to ``np = bc_np(n)``, a multiple of 32, identity on the padding;
  block k of ``nbk = np / 32`` is factored by one wave (``bc_diag_kernel``);
* ``below(k) = np / 16 - 2 (k + 1)`` 16-row tiles lie under block k.  With none (the last
  block; the only block at ``nbk = 1``) there is no panel and no update launch.  The panel
  runs ``ceil(below / 4)`` workgroups of four waves, one tile each: at ``below = 2`` half a
  workgroup returns at once;
* the update covers the ``ntl = below (below + 1) / 2`` lower tiles of the trailing matrix
  with ``min(1024, ceil(ntl / 4))`` workgroups of four waves: a wave takes a second tile
  only when ``ntl > 4096``, i.e. ``np >= 1504``, n >= 1473;
* ``bc_winv_kernel`` runs once per block row I >= 1, I workgroups each.

The polish kernel runs one workgroup per point: 16 waves (32 summation groups of 32
threads) while ``19 n`` doubles plus its static LDS fit ``kMaxLds``, 4 waves (8 groups) and
``7 n`` doubles past that.  ``mpo_trsm_f64`` gives a workgroup ``trsm_cols_per_block(n)``
right-hand sides, the most whose solutions fit the LDS.

Polish points never lie exactly on an observation: there the sign of the rounded
``amp - |v|^2`` decides between ``sd = 0`` (EI / PI answer 0, ``sd_g = 0``) and a tiny
positive sd, and no reference can say which way fp64 falls -- under a positive noise term.
Every point here has exact ``var_n >= 1e-6 amp`` (the host test fails if one does not -- no
point is ever dropped).  The kernel's ``sd <= 0`` branches run in
``tests/test_acq_sd_zero_gpu.py``, on models with a negative noise term
(``ps_cases.sd0_inputs``): there the variance at an observation is ``-amp`` or lower in every
precision and the inputs decide the branch.
"""
import functools
import math
from collections import namedtuple

import numpy as np

from tests import score_cases as S

K_BC = 32                    # kBc
K_MAX_LDS = S.K_MAX_LDS      # kMaxLds
K_MAX_OBS = S.K_MAX_OBS      # mpo::kMaxObs
UPDATE_GRID_CAP = 1024       # bc_update_kernel's grid cap
EXACT_MAX_N = S.EXACT_MAX_N  # the 80-bit references stop here; fp64 ones take over
EPS = S.EPS
AMP, NOISE = 2.0, 0.05
GRAD_BATCH_MAX = 65535       # mpo_gp_acq_grad's batch limit
SENTINEL = -7.25e77          # what the primitives' untouched entries are pre-filled with


# ---- the rules of gp.hip, restated ---------------------------------------------------
def bc_np(n):
    return (n + K_BC - 1) // K_BC * K_BC


def nbk(n):
    return bc_np(n) // K_BC


def below(n, k):
    """16-row tiles under diagonal block k."""
    return bc_np(n) // 16 - (k + 1) * 2


def panel_grid(n, k):
    """Workgroups of ``bc_panel_kernel`` after block k (0: not launched)."""
    b = below(n, k)
    return 0 if b <= 0 else (b + 3) // 4


def panel_idle_waves(n, k):
    """Waves of the panel launch that return on ``R >= np / 16``."""
    b = below(n, k)
    return 0 if b <= 0 else 4 * panel_grid(n, k) - b


def ntl(n, k):
    b = max(below(n, k), 0)
    return b * (b + 1) // 2


def update_grid(n, k):
    """Workgroups of ``bc_update_kernel`` after block k (0: not launched)."""
    if below(n, k) <= 0:
        return 0
    return max(1, min(UPDATE_GRID_CAP, (ntl(n, k) + 3) // 4))


def update_trips(n, k=0):
    """The most trips any wave of the update after block k takes through its tile loop."""
    g = update_grid(n, k)
    return 0 if g == 0 else -(-ntl(n, k) // (4 * g))


def tile_of(t):
    """``bc_update_kernel``'s decode of the linear lower-tile index t into (I, J), J <= I."""
    i = int((math.sqrt(8.0 * t + 1.0) - 1.0) * 0.5)
    while i * (i + 1) // 2 > t:
        i -= 1
    while (i + 1) * (i + 2) // 2 <= t:
        i += 1
    return i, t - i * (i + 1) // 2


def winv_launches(n):
    return [i for i in range(1, nbk(n))]


def trsm_cols_per_block(n):
    cb = 64
    while cb > 1 and n * cb * 8 > K_MAX_LDS - 1024:
        cb >>= 1
    return cb


pad_dims = S.pad_dims
np16_of = S.np16_of


def has_xb(n, d):
    """Whether ``mpo_gp_prepare`` builds the MFMA-distance rows: a resident model with two
    spare padded columns (MPO_GP_DIST and MPO_GP_SCORE unset)."""
    return S.plan(n, d)[0] == 0 and d + 2 <= pad_dims(d)


def polish_static_lds(nw):
    """``acq_grad_kernel<NW>``'s static LDS: red[64 NW] + ga, gu [2 NW][32] + xp[32] doubles."""
    return 8 * (64 * nw + 2 * (2 * nw) * 32 + 32)


def polish_waves(n):
    """16 or 4: the form ``mpo_gp_acq_grad`` launches (None: refused)."""
    if 19 * n * 8 + polish_static_lds(16) <= K_MAX_LDS:
        return 16
    return 4 if 7 * n * 8 + polish_static_lds(4) <= K_MAX_LDS else None


def polish_groups(n):
    """Summation groups of 32 threads in the gradient sums."""
    return 2 * polish_waves(n)


def polish_switch():
    """The largest n on the 16-wave form."""
    n = 1
    while polish_waves(n + 1) == 16:
        n += 1
    return n


# ---- prepare cases ----------------------------------------------------------------------
# kind: "well" (forward and backward bars), "ill" (backward only: cond(K) ~ 1e7),
#       "large" (past the 80-bit reference: fp64 reference, backward only)
Prep = namedtuple("Prep", "name n d noise kind reason")

PREPARE = [Prep(f"n{n}_d{d}", n, d, NOISE, "well", why) for n, d, why in [
    (1, 1, "one live row: nbk = 1, no panel, update or winv launch"),
    (2, 3, "nbk = 1, dp = 4 without xb"),
    (31, 5, "one short of a block, dp = 8 with xb"),
    (32, 10, "exactly one block, no padding, dp = 12 with xb"),
    (33, 12, "nbk = 2 with one live row in the second block; the panel runs half a workgroup"),
    (63, 32, "nbk = 2, one padded row, dp = 32"),
    (64, 16, "nbk = 2 exactly, dp = 16"),
    (65, 1, "nbk = 3: the first update with more than one tile row, a winv launch of 2 workgroups"),
    (96, 3, "nbk = 3 exactly"),
    (97, 5, "nbk = 4"),
    (545, 10, "nbk = 18: a ragged last block at the largest size the 80-bit factor takes"),
]]
PREPARE += [
    Prep("neardup_n120_d10", 120, 10, 1e-5, "ill", "60 pairs of observations 1e-4 apart at skopt's noise floor"),
    Prep("random_n96_d5", 96, 5, 1e-5, "ill", "96 random points at skopt's noise floor"),
    Prep("n1472_d4", 1472, 4, NOISE, "large", "np = 1472: ntl = 4095, the last size at which no update wave loops"),
    Prep("n1473_d4", 1473, 4, NOISE, "large", "np = 1504: ntl = 4278 > 4096, 182 waves take a second tile"),
    Prep("n2048_d4", 2048, 4, NOISE, "large", "the maximum: nbk = 64, ntl = 8001, two trips for all but 191 waves"),
]


def prep_by_name(name):
    return next(c for c in PREPARE if c.name == name)


def theta(d):
    """(amp, ls) of the append tests."""
    return AMP, np.linspace(0.5, 2.0, d)


@functools.lru_cache(maxsize=None)
def prep_inputs(name):
    """(X, y, amp, ls, noise) of a prepare case (read-only arrays)."""
    from oracle import gp_ei as O

    c = prep_by_name(name)
    if c.name.startswith("neardup"):
        # the problem of test_expanded_distance_small_noise_near_duplicates
        rng = np.random.RandomState(11)
        base = rng.uniform(size=(c.n // 2, c.d))
        X = np.concatenate([base, base + 1e-4 * rng.randn(c.n // 2, c.d)])
        y = np.sin(X @ rng.randn(c.d)) + 0.05 * rng.randn(c.n)
        amp, ls = 2.3, np.linspace(0.5, 1.6, c.d)
    else:
        X, y = O.synthetic_problem(c.n, c.d, seed=c.n + c.d)
        amp, ls = theta(c.d)
    for a in (X, y, ls):
        a.setflags(write=False)
    return X, y, amp, ls, c.noise


PrepRef = namedtuple("PrepRef", "st K L W alpha exact k_blk")


def block_factor(L):
    """``max_k || |L_kk^-1| |L_kk| ||_inf`` over the 32 x 32 diagonal blocks of a factor: the
    device multiplies by explicit block inverses (``D_k``), so its backward error carries
    this factor; substitution (LAPACK's ``trsm``) does not."""
    L = np.asarray(L, dtype=np.float64)
    worst = 1.0
    for k0 in range(0, L.shape[0], K_BC):
        B = L[k0:k0 + K_BC, k0:k0 + K_BC]
        worst = max(worst, float(np.max((np.abs(np.linalg.inv(B)) @ np.abs(B)).sum(1))))
    return worst


@functools.lru_cache(maxsize=None)
def prep_reference(name):
    """The reference of a prepare case, built once and shared (read-only): ``st`` the fp64
    state (scipy's factor), ``K`` the kernel matrix plus noise, and ``(L, W, alpha)`` -- of
    ``factor_exact`` in ``np.longdouble`` up to ``EXACT_MAX_N`` (``exact`` True), scipy's in
    fp64 past it."""
    from scipy.linalg import solve_triangular

    from oracle import gp_ei as O

    X, y, amp, ls, noise = prep_inputs(name)
    st = O.gp_from_theta(X, y, amp, ls, noise)
    n = X.shape[0]
    exact = n <= EXACT_MAX_N
    if exact:
        K = O.matern52_exact(X, X, ls, amp)
        K[np.diag_indices_from(K)] += np.longdouble(noise) + np.longdouble(O.SKOPT_ALPHA_JITTER)
        L, W, alpha = O.factor_exact(X, y, amp, ls, noise)
    else:
        K = O.matern52(X, X, ls, amp)
        K[np.diag_indices_from(K)] += noise + O.SKOPT_ALPHA_JITTER
        L, alpha = st.L, st.alpha
        W = solve_triangular(L, np.eye(n), lower=True, check_finite=False)
    for a in (K, L, W, alpha):
        a.setflags(write=False)
    return PrepRef(st, K, L, W, alpha, exact, block_factor(L))


def gamma(m):
    return m * EPS / (1.0 - m * EPS)


def backward_ratios(ref, L, W, amp):
    """(L ratio, W ratio): the largest residual / bound of a factor ``L`` and inverse ``W``
    (fp64 arrays) against a ``prep_reference``:

        |K_ref - L L^T|_ij <= 4 k_blk gamma_{n+1} (|L| |L^T|)_ij + 8 eps amp
        |W L - I|_ij       <= 4 k_blk gamma_n (|W| |L|)_ij

    Higham's Cholesky bound (Accuracy and Stability, thm 10.3) and the triangular-inverse
    residual (thm 14.1 applied row-wise) times the block factor, with 4 of headroom; the
    8 eps amp is K's own rounding (the kernel-matrix bar).  The products are formed in
    ``np.longdouble`` for an exact reference; in fp64 past it, where the gamma terms are
    doubled for the products' own rounding."""
    n = L.shape[0]
    t = np.longdouble if ref.exact else np.float64
    Lx, Wx = L.astype(t), W.astype(t)
    slack = 1.0 if ref.exact else 2.0
    bound_l = slack * 4 * ref.k_blk * gamma(n + 1) * (np.abs(L) @ np.abs(L).T) + 8 * EPS * amp
    res_l = np.abs(ref.K.astype(t) - Lx @ Lx.T)
    low = np.tril_indices(n)
    bound_w = slack * 4 * ref.k_blk * gamma(n) * (np.abs(W) @ np.abs(L))
    res_w = np.abs(Wx @ Lx - np.eye(n, dtype=t))
    # W L is lower triangular; above the diagonal residual and bound are both exactly 0
    ok = bound_w > 0
    assert np.all(res_w[~ok] == 0)
    return (float(np.max((res_l / bound_l)[low])), float(np.max(res_w[ok] / bound_w[ok])))


def forward_errors(ref, L, W, alpha):
    """The forward figures of test_device_factorisation_matches_oracle against the exact
    factor, each as a fraction of its bar: L at rtol 1e-11 / atol 1e-12, ``W L_x - I`` at
    1e-10, alpha at rtol 1e-8 / atol ``1e-10 max|alpha|``."""
    t = np.longdouble
    Lr, ar = ref.L.astype(t), ref.alpha.astype(t)
    e_l = float(np.max(np.abs(L.astype(t) - Lr) / (1e-11 * np.abs(Lr) + 1e-12)))
    e_w = float(np.max(np.abs(W.astype(t) @ Lr - np.eye(L.shape[0], dtype=t))) / 1e-10)
    d_a, tol_a = np.abs(alpha.astype(t) - ar), 1e-8 * np.abs(ar) + 1e-10 * np.max(np.abs(ar))
    # one observation: y_norm = 0, alpha = 0 and only the exact value passes
    e_a = float(np.max(np.where(tol_a > 0, d_a / np.where(tol_a > 0, tol_a, 1), np.where(d_a == 0, 0.0, np.inf))))
    return e_l, e_w, e_a


# ---- pivot-failure cases ------------------------------------------------------------------
# 70 points of a 4 x 4 x 5 lattice (spacings 0.25, 0.25, 0.2) at ls = 0.02: every off-diagonal
# is below 1e-7, and with amp = 2, noise = -1 every healthy pivot is 1 - O(1e-14).  Row j is a
# copy of row j - 1: K[j][j-1] = 2, so pivot j is 1 - 4 = -3.  Row j + 5 is a copy of row j + 4
# where it exists: a second, later failure that must not win.
Pivot = namedtuple("Pivot", "name n j noise second nan reason")
PIVOT_LS, PIVOT_AMP = 0.02, 2.0

PIVOT = [Pivot(f"dup_j{j}", 70, j, -1.0, j + 5 < 70, False, why) for j, why in [
    (1, "the second column of the first block"),
    (31, "the last column of a block"),
    (32, "the first column of the second block"),
    (33, "inside the second block"),
    (63, "the last column of the second block; the later failure is in the third"),
    (64, "the first column of the ragged third block"),
    (69, "the last live row; the padded identity rows after it must not report"),
]]
PIVOT += [
    Pivot("noise_col0", 70, 0, -3.0, False, False, "noise = -3: the very first pivot is -1"),
    Pivot("n33_j32", 33, 32, -1.0, False, False, "the single live row of a padded block"),
    Pivot("nan_j33", 70, 33, -1.0, True, True, "a NaN coordinate in row 33: the !isfinite branch, and a later "
          "duplicate"),
]


def pivot_by_name(name):
    return next(c for c in PIVOT if c.name == name)


def lattice(n):
    g4, g5 = 0.1 + 0.25 * np.arange(4), 0.1 + 0.2 * np.arange(5)
    P = np.array([(a, b, c) for a in g4 for b in g4 for c in g5])
    return P[:n].copy()


@functools.lru_cache(maxsize=None)
def pivot_inputs(name):
    """(X, y, amp, ls, noise) of a pivot-failure case."""
    c = pivot_by_name(name)
    X = lattice(c.n)
    if c.nan:
        X[c.j, 1] = np.nan
    elif c.j > 0:
        X[c.j] = X[c.j - 1]
    if c.second:
        X[c.j + 5] = X[c.j + 4]
    y = np.sin(7.0 * np.arange(c.n))
    ls = np.full(3, PIVOT_LS)
    for a in (X, y, ls):
        a.setflags(write=False)
    return X, y, PIVOT_AMP, ls, c.noise


def pivot_matrix(name):
    """The fp64 kernel matrix plus noise of a pivot-failure case (what ``mpo_chol_f64`` is fed)."""
    from oracle import gp_ei as O

    X, _, amp, ls, noise = pivot_inputs(name)
    with np.errstate(invalid="ignore"):
        K = O.matern52(X, X, ls, amp)
    K[np.diag_indices_from(K)] += noise + O.SKOPT_ALPHA_JITTER
    return K


# ---- polish cases ---------------------------------------------------------------------------
Polish = namedtuple("Polish", "name n d reason")
POLISH_B = 19


def _polish_cases():
    lo = polish_switch()
    rows = [
        (1, 1, "one observation, one dimension: 1023 idle threads, every group but one empty"),
        (2, 2, "fewer observations than waves"),
        (15, 32, "n below the 16 waves at d = 32: tid < 32 fills xp, tid & 31 indexes every ga / gu column"),
        (17, 4, "one wave takes a second row of W"),
        (33, 5, "one summation group takes a second observation"),
        (63, 31, "d = 31: one idle gradient column; one short of a wave's lanes"),
        (64, 10, "a row of W exactly one wave wide"),
        (65, 12, "a row of W one past a wave: the c += 64 trip"),
        (129, 8, "two c += 64 trips"),
        (lo, 3, f"the last n on the 16-wave form ({19 * lo * 8 + polish_static_lds(16)} of {K_MAX_LDS} bytes)"),
        (lo + 1, 3, "the first n on the 4-wave form"),
        (K_MAX_OBS, 8, "the maximum, 4 waves"),
    ]
    return [Polish(f"n{n}_d{d}", n, d, why) for n, d, why in rows]


POLISH = _polish_cases()
SWITCH = (POLISH[-3], POLISH[-2])


def polish_by_name(name):
    return next(c for c in POLISH if c.name == name)


@functools.lru_cache(maxsize=None)
def polish_inputs(name):
    """(X, y, amp, ls, noise, P, y_opt): the model and the B = 19 points of one launch -- 12
    uniform draws, the corners 0 and 1, 3 observations shifted by 1e-3 in every coordinate
    and 2 mid-points of observation pairs.  With fewer than 3 observations the shifted ones
    repeat with 2e-3, 3e-3; with fewer than 4 the second "mid-point" is the quarter point of
    the first pair, and with a single observation both pair it with a corner (a mid-point
    of an observation with itself would lie on it).  ``y_opt`` is the median target, not the
    best one: z = (y_opt - xi - mu) / sd then takes both signs and stays inside +-38 at nearly
    every point, where with the minimum EI and PI underflow to 0 at most points of the dense
    models (z down to -128 at n = 915) and their bars would hold vacuously.  The minimum runs
    in ``tests/test_acq_ps_edges_gpu.py``, which asserts exact zeros at the underflowed points."""
    from oracle import gp_ei as O

    c = polish_by_name(name)
    X, y = O.synthetic_problem(c.n, c.d, seed=c.n + c.d)
    amp, ls = theta(c.d)
    rng = np.random.RandomState(1000 + c.n + c.d)
    shifted = [X[i % c.n] + 1e-3 * (1 + i // c.n) for i in range(3)]
    if c.n >= 4:
        mids = [0.5 * (X[0] + X[1]), 0.5 * (X[2] + X[3])]
    elif c.n >= 2:
        mids = [0.5 * (X[0] + X[1]), 0.25 * X[0] + 0.75 * X[1]]
    else:
        mids = [0.5 * X[0], 0.5 * (X[0] + 1.0)]
    P = np.vstack([rng.uniform(size=(12, c.d)), np.zeros(c.d), np.ones(c.d)] + shifted + mids)
    assert P.shape == (POLISH_B, c.d)
    for a in (X, y, ls, P):
        a.setflags(write=False)
    return X, y, amp, ls, NOISE, P, float(np.median(y))


PolishRef = namedtuple("PolishRef", "st exact mu sd mu_g sd_g mu_scale mu_g_scale sd_g_scale var_n tri_err bars")
POLISH_BAR = 1e-9


def polish_errors(r, mu, sd, mu_g, sd_g):
    """The four error figures of a posterior and its gradients at the B points against the
    reference ``r``: mu relative to its summand scale (as test_gp_gpu.py's ``mu_scale``), sd
    relative, ``mu_g[j]`` relative to ``y_std sum_i |dk_ij| |alpha_i|``, ``sd_g[j]`` relative
    to ``y_std sum_i |dk_ij| (|W|^T |W| |k*|)_i / sd_n + |sd_g[j]|``."""
    t = np.longdouble

    def worst(got, want, scale):
        # a zero scale (alpha = 0 with one observation) admits only the exact value
        diff = np.abs(np.asarray(got, t) - want)
        safe = np.where(scale > 0, scale, 1.0)
        return float(np.max(np.where(scale > 0, diff / safe, np.where(diff == 0, 0.0, np.inf))))

    return (worst(mu, r.mu, r.mu_scale), worst(sd, r.sd, r.sd.astype(np.float64)),
            worst(mu_g, r.mu_g, r.mu_g_scale), worst(sd_g, r.sd_g, r.sd_g_scale))


@functools.lru_cache(maxsize=None)
def polish_reference(name):
    """The reference of a polish case at its B points, built once and shared:
    ``posterior_grad_exact`` up to ``EXACT_MAX_N`` observations, ``posterior_grad_tri64``
    past it; the scales of the four error figures; the exact normalised variance; and
    the bars -- ``max(1e-9, 4 x posterior_grad_tri64's own error)`` per figure where the
    exact reference runs (``tri_err``), the plain 1e-9 past it."""
    from scipy.linalg import solve_triangular

    from oracle import gp_ei as O

    X, y, amp, ls, noise, P, _ = polish_inputs(name)
    st = O.gp_from_theta(X, y, amp, ls, noise)
    n = X.shape[0]
    exact = n <= EXACT_MAX_N
    W64 = solve_triangular(st.L, np.eye(n), lower=True, check_finite=False)
    tri = [O.posterior_grad_tri64(st, x, W64) for x in P]
    if exact:
        fx = O.factor_exact(X, y, amp, ls, noise)
        ref = [O.posterior_grad_exact(st, x, fx) for x in P]
        W, alpha = np.abs(fx[1]).astype(np.float64), np.abs(fx[2]).astype(np.float64)
    else:
        ref = tri
        W, alpha = np.abs(W64), np.abs(st.alpha)
    t = np.longdouble
    mu, sd = np.array([r[0] for r in ref], dtype=t), np.array([r[1] for r in ref], dtype=t)
    mu_g, sd_g = np.array([r[2] for r in ref], dtype=t), np.array([r[3] for r in ref], dtype=t)
    # scales, from the fp64 kernel row and its derivative
    Ks = np.abs(O.matern52(P, X, ls, amp))                                # [B][n]
    mu_scale = st.y_std * (Ks @ alpha) + abs(st.y_mean)
    diff = P[:, None, :] - X[None, :, :]                                  # [B][n][d]
    tt = O.SQRT5 * np.sqrt(np.sum((diff / ls) ** 2, axis=2))
    dk = np.abs((5.0 / 3.0) * amp * ((1.0 + tt) * np.exp(-tt))[:, :, None] * diff / ls ** 2)
    sd_n = (sd / t(st.y_std)).astype(np.float64)
    mu_g_scale = st.y_std * np.einsum("bnd,n->bd", dk, alpha)
    wwk = (Ks @ W.T) @ W                                                   # (|W|^T |W| |k*|) per point
    sd_g_scale = st.y_std * np.einsum("bnd,bn->bd", dk, wwk) / sd_n[:, None] + np.abs(sd_g).astype(np.float64)
    var_n = sd_n ** 2
    r = PolishRef(st, exact, mu, sd, mu_g, sd_g, mu_scale, mu_g_scale, sd_g_scale, var_n, None, None)
    if exact:
        tri_err = polish_errors(r, *(np.array([q[i] for q in tri]) for i in range(4)))
        bars = tuple(max(POLISH_BAR, 4.0 * e) for e in tri_err)
    else:
        tri_err, bars = None, (POLISH_BAR,) * 4
    return r._replace(tri_err=tri_err, bars=bars)


def extract_posterior(f0, fk, g0, gk, kappa):
    """(mu, sd, mu_g, sd_g) from two LCB launches, kappa = 0 and kappa = a power of two:
    ``mu = f_0``, ``sd = (f_0 - f_k) / kappa`` and likewise the gradients.  The scaling is
    exact, so the extraction costs ``eps (|mu| / kappa + sd)``."""
    return f0, (f0 - fk) / kappa, g0, (g0 - gk) / kappa


POLISH_KAPPA = 2.0 ** 30


# ---- primitive cases -------------------------------------------------------------------------
KMAT = [(1, 1, 1), (63, 1, 63), (64, 5, 70), (65, 32, 65)]          # (n, d, ldk)
KMAT_DIAG = (0.0, 0.05 + 1e-10)
CHOL_N = (1, 2, 63, 64, 65, 1026)                                    # lda = n and n + 3 each
CHOL_PAD = 3
CHOL_THREADS = 1024                                                  # chol_kernel's block: i += nt loops past it
TRSM_N = (1, 65, 318, 319)
TRSM_PAD = 5


def trsm_nrhs(n):
    cb = trsm_cols_per_block(n)
    return [1, cb - 1, cb, cb + 1] if cb > 2 else [1, cb, cb + 1]


@functools.lru_cache(maxsize=None)
def spd_matrix(n, d=8):
    """A well-conditioned kernel matrix plus noise for the Cholesky and the solve (fp64)."""
    from oracle import gp_ei as O

    X, _ = O.synthetic_problem(n, d, seed=3 * n + d)
    amp, ls = theta(d)
    K = O.matern52(X, X, ls, amp)
    K[np.diag_indices_from(K)] += NOISE + O.SKOPT_ALPHA_JITTER
    K.setflags(write=False)
    return K


def kmat_inputs(n, d):
    from oracle import gp_ei as O

    X, _ = O.synthetic_problem(n, d, seed=5 * n + d)
    return X, theta(d)[1]
