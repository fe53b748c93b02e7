"""Inputs of the joint-posterior tests (tests/test_gp_joint_gpu.py), importable by the test
and runnable as a script in a fresh process:

    python tests/joint_cases.py OUT.npz

writes the covariance and the samples of ``PATH_CASE`` as the device computes them under
the environment of that process (``MPO_GP_SCORE=streamed`` is read at prepare time).

The inputs are those of the other GP tests: ``O.synthetic_problem(n, d, seed=n + d)``,
theta = (2.0, linspace(0.5, 2, d), 0.05), ``O.synthetic_candidates(m, d, seed=7)`` and
``Z = RandomState(3).standard_normal((m, s))``.

Below the inputs: a plain-Python restatement of the launch geometry of ``csrc/gp_joint.hip``
(named after the source), the table ``CASES`` of the shapes at which that geometry changes
(run by ``tests/test_gp_joint_shapes_gpu.py``, guarded by ``tests/test_joint_cases_host.py``)
and the references those shapes are judged against.  No GPU or torch import at module level.

What decides how a call is launched:

* ``mp = joint_mp(m)``, m rounded up to 32 with identity on the padding; ``np16``, n rounded
  up to 16;
* ``joint_v_kernel`` runs ``v_grid(n, m) = (mp / 16, ceil(np16 / 256))`` workgroups.  Workgroup
  (ct, J) owns the columns [256 J, 256 J + 256) of V and walks the K* panels 0 .. J; its wave
  w owns the column tiles j0 = 256 J + 16 (4 w + q) and runs ``lim[q]`` k-steps of panel p,
  none where j0 >= np16.  Only the workgroups of the last J sum mu;
* ``joint_cov_kernel`` deals the ``cov_tiles(rows)`` lower 16 x 16 tiles round-robin over
  ``cov_grid(rows)`` <= 2048 workgroups of four waves, so a wave takes a second tile from
  rows = 2033 on (``cov_trips``).  rows = m for the public covariance, mp for the matrix that
  is factored;
* ``mpo::blocked_chol`` factors that mp x mp matrix with the block steps of ``mpo_gp_prepare``
  (``factor_cases``): ``chol_update_trips(mp)`` trips of ``bc_update_kernel`` after block 0;
* ``joint_sample_kernel`` runs ``sample_grid(m, s) = (ceil(mp / 64), ceil(s / 16))`` workgroups,
  one 16-row tile per wave.  ``sample_idle_waves(m)`` waves of the last workgroup have no tile
  and enter the argmin fold with (inf, LLONG_MAX);
* ``argmin_fold_kernel`` (``mpo::argmin_fold``) runs ``argmin_blocks(s)`` workgroups of 256 draws.
"""
import functools
import os
import sys
from collections import namedtuple

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


# ---- the rules of gp_joint.hip, restated -------------------------------------------------
from tests import factor_cases as F  # noqa: E402

LD = np.longdouble
EPS = F.EPS
JOINT_MAX = 4096             # MPO_JOINT_MAX
JOINT_SMAX = 1048560         # MPO_JOINT_SMAX = 16 x 65535
K_PANEL = 256                # kPanel
COV_GRID_CAP = 2048          # joint_cov_kernel's grid cap
EXACT_MAX = F.EXACT_MAX_N    # the end-to-end 80-bit chain stops at n, m <= 600
ROWS_80BIT_MAX = 2048        # the m x m Matern in np.longdouble stops here; fp64 past it

pad_dims = F.pad_dims
np16_of = F.np16_of
gamma = F.gamma


def joint_mp(m):
    return (m + 31) // 32 * 32


def joint_nb(m):
    return (joint_mp(m) + 63) // 64


def v_grid(n, m):
    """Workgroups (x, y) of ``joint_v_kernel``: query tiles x panels of 256 columns of V."""
    return joint_mp(m) // 16, (np16_of(n) + K_PANEL - 1) // K_PANEL


def v_lim(n, J, wave, p):
    """``lim[q]``, q = 0..3, of wave ``wave`` in a workgroup of panel column J at K* panel p."""
    np_, i0 = np16_of(n), p * K_PANEL
    out = []
    for q in range(4):
        j0 = J * K_PANEL + 16 * (4 * wave + q)
        out.append(min(K_PANEL, j0 + 16 - i0) // 4 if j0 < np_ else 0)
    return out


def v_live_tiles(n, J, wave):
    """Column tiles of V that wave ``wave`` of panel column J computes and stores: the q whose
    ``lim[q]`` is not 0 at the wave's last panel p = J."""
    return sum(1 for k in v_lim(n, J, wave, J) if k > 0)


def cov_tiles(rows):
    t = (rows + 15) // 16
    return t * (t + 1) // 2


def cov_grid(rows):
    return max(1, min(COV_GRID_CAP, (cov_tiles(rows) + 3) // 4))


def cov_trips(rows):
    """The most trips any wave of ``joint_cov_kernel`` takes through its tile loop."""
    return -(-cov_tiles(rows) // (4 * cov_grid(rows)))


def cov_last_trip_waves(rows):
    """How many waves take that last trip."""
    nw = 4 * cov_grid(rows)
    return cov_tiles(rows) - (cov_trips(rows) - 1) * nw


def sample_grid(m, s):
    return joint_nb(m), (s + 15) // 16


def sample_idle_waves(m):
    """Waves of ``joint_sample_kernel``'s last workgroup with ``i0 >= mp``."""
    return 4 * joint_nb(m) - joint_mp(m) // 16


def argmin_blocks(s):
    return (s + 255) // 256


def chol_update_trips(mp, k=0):
    """``bc_update_kernel``'s trips after block k of the mp x mp factorisation."""
    assert mp % 32 == 0
    return F.update_trips(mp, k)


# ---- the case table ------------------------------------------------------------------------
# what: "cov" (mpo_gp_posterior_cov: covariance, mu, sd) or "sample" (that, then mpo_gp_sample
# twice: Z = I for the factor, Z of inputs() for the samples and the argmin).  s = 0 with "cov".
Case = namedtuple("Case", "name n d m s what why")
S_LARGE = 16                 # draws of the cases past the 80-bit chain


def _cases():
    rows = []
    # V panels: covariance + mu at small m
    for n, why in [
        (255, "np16 = 256: the last single-panel n with a dead observation slot (obs < n) in the K* panel"),
        (256, "np16 = 256: one full panel, v_grid y = 1, every wave four live tiles, mu on J = 0"),
        (257, "np16 = 272: v_grid y = 2; at J = 1 wave 0 has one live tile (lim = [4, 0, 0, 0] at p = 1), waves "
              "1-3 none; mu only on J = 1; W's row 257..271 guard (j < n)"),
        (512, "np16 = 512: two full panels, every lim at its cap of 64 k-steps on p = 0"),
        (513, "np16 = 528: v_grid y = 3, the second single-tile panel"),
    ]:
        rows.append((f"v_n{n}", n, 4, 17, 0, "cov", why))
    rows.append(("v_n2048", 2048, 4, 32, 0, "cov", "the maximum n: v_grid y = 8, eight K* panels, mu on J = 7 only"))
    for d, why in [(1, "dp = 4: three zero columns"), (5, "dp = 8: three zero columns"), (32, "dp = 32: none")]:
        rows.append((f"v_d{d}", 33, d, 17, 0, "cov", why + "; mp = 32 with 15 repeated query rows"))
    # the tile loop of joint_cov_kernel
    rows += [
        ("cov_m2032", 16, 10, 2032, 0, "cov", "rows = 2032: cov_tiles = 8128 <= 8192 waves, cov_trips = 1 (the last)"),
        ("cov_m2033", 16, 10, 2033, 0, "cov", "rows = 2033: cov_tiles = 8256, cov_trips = 2, 64 waves take a second "
         "tile (the ragged tile row 127)"),
        ("sample_m2016", 16, 10, 2016, S_LARGE, "sample", "mp = 2016: the factored matrix in one trip (8001 tiles); "
         "chol_update_trips = 2"),
        ("sample_m2017", 16, 10, 2017, S_LARGE, "sample", "mp = 2048: the factored matrix takes cov_trips = 2 on "
         "exactly 64 tiles -- the default Thompson ask's shape"),
        ("cov_m4096", 16, 10, 4096, 0, "cov", "the maximum m: cov_tiles = 32896, cov_trips = 5, 128 waves take the "
         "fifth"),
        ("sample_m4096", 16, 10, 4096, S_LARGE, "sample", "the maximum: mp = 4096, chol_update_trips = 8 at k = 0, "
         "sample_grid x = 64"),
    ]
    # joint_sample_kernel's geometry
    for m, why in [
        (1, "mp = 32: one workgroup, sample_idle_waves = 2, 31 identity rows"),
        (32, "mp = 32 exactly: sample_idle_waves = 2, no padding"),
        (33, "mp = 64: the first full workgroup, 31 identity rows"),
        (64, "mp = 64 exactly: sample_idle_waves = 0"),
        (65, "mp = 96: two workgroups, the second with one idle wave; the first two-partial fold"),
    ]:
        rows.append((f"sample_m{m}", 16, 10, m, 16, "sample", why + "; sample_grid y = 1, exactly 16 draws"))
    rows += [
        ("sample_s256", 16, 10, 33, 256, "sample", "argmin_blocks = 1 with every thread live; sample_grid y = 16"),
        ("sample_s257", 16, 10, 33, 257, "sample", "argmin_blocks = 2: one draw in the second block; sample_grid "
         "y = 17 with 15 dead draw columns (r < s)"),
        ("const_y", 16, 4, 17, 16, "sample", "all targets equal: y_std -> 1, alpha = 0, mu = y_mean exactly"),
        ("sample_smax", 16, 10, 1, JOINT_SMAX, "sample", "s = MPO_JOINT_SMAX: sample_grid y = 65535, the widest; "
         "argmin_blocks = 4096"),
    ]
    return [Case(*r) for r in rows]


CASES = _cases()
CONST_Y = 1.25               # the targets of const_y


def case_by_name(name):
    return next(c for c in CASES if c.name == name)


def is_exact(c):
    """Whether the end-to-end 80-bit chain is the case's reference."""
    return c.n <= EXACT_MAX and c.m <= EXACT_MAX


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(X, y, C, Z) of a case: those of ``inputs`` (read-only arrays)."""
    c = case_by_name(name)
    X, y, C, Z = inputs(c.n, c.d, c.m, c.s)
    if name == "const_y":
        y = np.full(c.n, CONST_Y)
    for a in (X, y, C, Z):
        if a is not None:
            a.setflags(write=False)
    return X, y, C, Z


def normalise(y):
    y_mean, y_std = float(np.mean(y)), float(np.std(y))
    return y_mean, (y_std if y_std != 0.0 else 1.0)


# ---- references ------------------------------------------------------------------------------
def posterior_from_factor(X, C, ls, amp, W, alpha, y_mean, y_std, t=LD, rows=None):
    """The joint posterior from a factor's ``W = L^-1`` and ``alpha`` (any source: the exact
    chain's, scipy's, or the device's own -- then the joint kernels are judged alone) in the
    number type ``t``: ``np.longdouble`` with ``matern52_exact``, or ``np.float64`` with the
    oracle's fp64 ``matern52`` (the restatement used where the m x m Matern in 80-bit is too
    slow).  ``rows``: only those rows of Sigma_n (all columns).

    Returns a dict: Sn (Sigma_n = amp Matern52(c, c) - V V^T), mu, mu_scale (the summand scale
    of the mu bar) and QQ = Q Q^T with Q = |K*| |W^T|, the scale of the derived bound."""
    if t is LD:
        Ks = O.matern52_exact(C, X, ls, amp)
        Wt, at = np.asarray(W).astype(LD), np.asarray(alpha).astype(LD)
    else:
        Ks = O.matern52(C, X, ls, amp)
        Wt, at = np.asarray(W, dtype=np.float64), np.asarray(alpha, dtype=np.float64)
    V = Ks @ Wt.T
    Q = np.abs(Ks).astype(np.float64) @ np.abs(Wt).astype(np.float64).T
    sel = slice(None) if rows is None else np.asarray(rows)
    Kcc = O.matern52_exact(C[sel], C, ls, amp) if t is LD else O.matern52(C[sel], C, ls, amp)
    Sn = Kcc - V[sel] @ V.T
    mu = t(y_mean) + t(y_std) * (Ks @ at)
    mu_scale = (y_std * (np.abs(Ks) @ np.abs(at)) + abs(y_mean)).astype(np.float64)
    return {"Sn": Sn, "mu": mu, "mu_scale": mu_scale, "QQ": Q[sel] @ Q.T, "y_std": y_std, "amp": amp,
            "rows": rows, "n": X.shape[0]}


def exact_chain_of(X, y, C, Z, d, jitter=JITTER):
    """The end-to-end 80-bit chain: ``factor_exact`` -> ``posterior_from_factor`` -> (with a Z)
    ``cholesky_exact`` of Sigma_n + jitter amp I and the samples."""
    amp, ls, noise = theta(d)
    _, W, alpha = O.factor_exact(X, y, amp, ls, noise)
    y_mean, y_std = normalise(y)
    r = posterior_from_factor(X, C, ls, amp, W, alpha, y_mean, y_std)
    if Z is not None:
        m = C.shape[0]
        Lc, info = O.cholesky_exact(r["Sn"] + LD(jitter) * LD(amp) * np.eye(m, dtype=LD))
        assert info == 0
        r["Lc"] = Lc
        r["S"] = r["mu"][None, :] + LD(y_std) * (Lc @ Z.astype(LD)).T
    return r


@functools.lru_cache(maxsize=None)
def exact_chain(name):
    """The 80-bit reference of an ``is_exact`` case, shared between the tests: never written."""
    c = case_by_name(name)
    assert is_exact(c)
    return exact_chain_of(*case_inputs(name), c.d)


def fp64_chain(X, y, C, Z, d, jitter=JITTER):
    """The whole chain in fp64 (scipy's factor, LAPACK's Cholesky): the host guard's stand-in
    for the device.  Returns (posterior dict, Lc, samples, info)."""
    from scipy.linalg import solve_triangular
    from scipy.linalg.lapack import dpotrf

    amp, ls, noise = theta(d)
    st = O.gp_from_theta(X, y, amp, ls, noise)
    W = solve_triangular(st.L, np.eye(st.n), lower=True, check_finite=False)
    r = posterior_from_factor(X, C, ls, amp, W, st.alpha, st.y_mean, st.y_std, t=np.float64)
    A = r["Sn"] + jitter * amp * np.eye(C.shape[0])
    Lc, info = dpotrf(A, lower=1)
    Lc = np.tril(Lc)
    S = None if (info or Z is None) else r["mu"][None, :] + st.y_std * (Lc @ Z).T
    return r, Lc, S, info


def tile_rows(m):
    """One row per 16-row tile row I, at offset (7 I) mod 16 (the last one clipped to m - 1):
    with all columns, and the mirror, every 16 x 16 tile of the covariance is touched."""
    return np.array([min(16 * i + (7 * i) % 16, m - 1) for i in range((m + 15) // 16)])


def cov_bound(r):
    """The derived entrywise bound on |Sigma_n(device) - Sigma_n|: V = K* W^T carries
    gamma_n |K*| |W^T| = gamma_n Q (plus K*'s own few eps, relative), the tile's product over
    np16 k-steps gamma_np16 |V| |V^T| <= gamma_np16 Q Q^T, twice the first in the product, the
    Matern and the subtraction a few eps amp:

        4 (2 gamma_{n + np16 + 8} (Q Q^T)_ij + 8 eps amp)."""
    n = r["n"]
    return 4.0 * (2.0 * gamma(n + np16_of(n) + 8) * r["QQ"] + 8.0 * EPS * r["amp"])


def factor_ratio(A, Lc, amp, exact_product):
    """The largest |A - Lc Lc^T|_ij over its bound, ``factor_cases.backward_ratios``' L bound
    on the mp x mp factorisation:

        4 k_blk gamma_{mp+1} (|Lc| |Lc^T|)_ij + 8 eps amp,

    k_blk = ``block_factor(Lc)``.  The product in ``np.longdouble`` where affordable; in fp64
    past it, where the gamma term is doubled for the product's own rounding.  Returns
    (ratio, k_blk, largest residual)."""
    m = Lc.shape[0]
    k_blk = F.block_factor(Lc)
    t = LD if exact_product else np.float64
    slack = 1.0 if exact_product else 2.0
    L64 = np.asarray(Lc, dtype=np.float64)
    bound = slack * 4 * k_blk * gamma(joint_mp(m) + 1) * (np.abs(L64) @ np.abs(L64).T) + 8 * EPS * amp
    Lt = L64.astype(t)
    res = np.abs(np.asarray(A).astype(t) - Lt @ Lt.T)
    return float(np.max(res / bound)), k_blk, float(np.max(res))


ARGMIN_GAP = 1e-6            # of y_std sqrt(amp): below it a draw's argmin is judged by value
VALUE_BAR = 1e-9


def argmin_check(S_ref, am, scale):
    """The argmin rule of test_thompson_gpu.py: exact where the reference's best-to-second gap
    exceeds ``ARGMIN_GAP`` of the scale, by value at 1e-9 otherwise.  Returns (ok per draw,
    draws judged by value)."""
    S_ref = np.asarray(S_ref)
    s, m = S_ref.shape
    best = np.argmin(S_ref, axis=1)
    if m == 1:
        return am == 0, 0
    part = np.partition(S_ref, 1, axis=1)
    by_value = (part[:, 1] - part[:, 0]) <= ARGMIN_GAP * scale
    picked = S_ref[np.arange(s), np.clip(am, 0, m - 1)]
    ok = np.where(by_value, (picked - part[:, 0]) <= VALUE_BAR * scale, am == best)
    return ok & (am >= 0) & (am < m), int(np.sum(by_value))


# ---- argmin placement and ties ---------------------------------------------------------------
# Z = 0: every draw equals mu, so the candidate of lowest mu, c*, is the argmin wherever it is
# put.  m = 200: mp = 224, sample_grid x = 4, the last workgroup with two live waves.
PLACE_N, PLACE_D, PLACE_M = 64, 4, 200
PLACE_JITTER = 1e-4          # duplicates make Sigma_n singular; with Z = 0 only a finite Lc matters
PLACE_S = 17
PLACE_SINGLE = (0, 3, 4, 15, 16, 63, 64, 191, 192, 199)
PLACE_DUP = (
    (0, 4, "the same lane, another q: the in-lane fold"),
    (0, 1, "neighbouring rows of one q: the butterfly over lane >> 4"),
    (3, 16, "another lane group and another wave"),
    (15, 16, "the last row of wave 0 and the first of wave 1: the LDS fold"),
    (63, 64, "across workgroups: the partial fold"),
    (64, 128, "workgroups 1 and 2: the partial fold's order"),
    (0, 199, "the first and the last row"),
    (192, 199, "both in the last workgroup's first wave"),
)


@functools.lru_cache(maxsize=None)
def placement_pool():
    """(X, y, pool, index of c*, fp64 mu of the pool): the model of ``PATH_CASE`` and the
    seed-7 pool of 200 candidates."""
    X, y, pool, _ = inputs(PLACE_N, PLACE_D, PLACE_M)
    amp, ls, noise = theta(PLACE_D)
    st = O.gp_from_theta(X, y, amp, ls, noise)
    mu = st.y_mean + st.y_std * (O.matern52(pool, X, ls, amp) @ st.alpha)
    for a in (X, y, pool, mu):
        a.setflags(write=False)
    return X, y, pool, int(np.argmin(mu)), mu


def placement_candidates(i1, i2=None):
    """The 200 candidates with c* at index i1 (and a second copy at i2 > i1): the rest of the
    pool in its order, its last point dropped for the copy."""
    _, _, pool, star, _ = placement_pool()
    others = np.delete(pool, star, axis=0)
    if i2 is None:
        return np.insert(others, i1, pool[star], axis=0)
    assert i1 < i2
    C = np.insert(others[:-1], i1, pool[star], axis=0)
    return np.insert(C, i2, pool[star], axis=0)


# ---- failure reporting past the first block ---------------------------------------------------
FAIL_AT, FAIL_AGAIN = 40, 45


def failure_inputs(second):
    """(X, y, ls, queries): the one-observation model of test_failed_factor_reports_the_column
    (amp = 2, noise = -1: Sigma_n = 2 - 4 at the observation itself) and 70 queries on
    ``factor_cases.lattice`` at its length scale, the observation being lattice point 40 (and
    a copy of it at index 45 when ``second``).  Every other query is ten length scales away:
    its pivot is 2 - O(1e-14)."""
    Q = F.lattice(70)
    if second:
        Q[FAIL_AGAIN] = Q[FAIL_AT]
    return Q[FAIL_AT:FAIL_AT + 1].copy(), np.array([1.0]), np.full(3, F.PIVOT_LS), Q


# ---- the C ABI ---------------------------------------------------------------------------------
ABI_CASE = (33, 32, 80, 17)  # (n, d, m, s)
ABI_PAD = 3                  # ldc = m + 3
GUARD_BYTES = 4096


if __name__ == "__main__":
    n, d, m, s = PATH_CASE
    X, y, C, Z = inputs(n, d, m, s)
    g = device_gp(X, y, d)
    mu, cov, samples, argmin, info = device_joint(g, C, Z)
    np.savez(sys.argv[1], mu=mu, cov=cov, samples=samples, argmin=argmin, info=info, score_path=g.score_path)
