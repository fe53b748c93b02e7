"""The fixtures of the cost-aware acquisition tests (tests/test_acq_ps_gpu.py): model pairs and
points rebuilt from seeds, and their 80-bit references, computed once on the CPU by
``python -m tests.ps_cases`` (minutes: the exact factors at n = 914, 915 and 1300) and kept in
``tests/golden/acq_ps_ref.npz``.  No GPU or torch import.

The edge fixtures (tests/test_acq_sd_zero_gpu.py, tests/test_acq_ps_edges_gpu.py; guarded on the
CPU by tests/test_acq_ps_edges_host.py): ``sd0_inputs`` -- models under a negative noise term whose
posterior variance at every observation is negative, so the kernels' ``sd <= 0`` branches are
decided by the inputs -- and the ``y_opt`` the search itself passes, ``min(y)``, and lower, where
EI and PI underflow at part of the candidates; their references are computed by
``python -m tests.ps_cases edges`` into ``tests/golden/acq_ps_edges_ref.npz``.
"""
import functools
import os

import numpy as np

from oracle import gp_ei as O
from tests import ps_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "acq_ps_ref.npz")
LD = np.longdouble
XI = 0.01
TOPK = 5
#: (n, d, m) of the scoring parity; the last model is past the LDS-resident limit (streamed)
SCORE = [(1, 1, 1), (17, 3, 65), (40, 5, 257), (200, 10, 4096), (1300, 4, 64)]
#: (n, d) of the gradient parity: 914 / 915 are the two sides of the kernel's 16 / 4-wave switch
#: ((19 n + 3104) doubles <= 160 KiB: the static LDS is mpo_gp_acq_grad's kernel's)
GRAD = [(1, 1), (17, 5), (200, 10), (914, 32), (915, 5)]
GRAD_B = 15
ACQS = ("EI", "PI")


def inputs(n, d):
    """``(X, y, logt, theta_f, theta_t, y_opt)``: the oracle's synthetic objective, log-times
    that vary over an order of magnitude, two different sets of hyper-parameters.  ``y_opt``
    is the median value: z takes both signs and EI and PI underflow nowhere, so every point of
    the ``SCORE`` / ``GRAD`` tables has a bar that binds.  The minimum -- what the optimizer
    passes -- and values below it, where part of the points underflow to exact zeros, are the
    ``EDGE_*`` cases further down."""
    X, y = O.synthetic_problem(n, d, seed=100 + n + d)
    rng = np.random.RandomState(200 + n + d)
    logt = 1.2 * np.sin(X @ rng.randn(d)) + 0.8 * X[:, 0] + 0.05 * rng.randn(n) + 0.5
    ls_f = 0.45 + 0.11 * (np.arange(d) % 5)
    ls_t = 0.95 - 0.07 * (np.arange(d) % 4)
    for a in (X, y, logt, ls_f, ls_t):
        a.setflags(write=False)
    return X, y, logt, (1.3, ls_f, 0.02), (0.8, ls_t, 0.05), float(np.median(y))


@functools.lru_cache(maxsize=None)
def pair(n, d):
    """The two reference models of ``inputs(n, d)`` (shared; their factors are built lazily)."""
    X, y, logt, th_f, th_t, _ = inputs(n, d)
    return R.Model(X, y, *th_f), R.Model(X, logt, *th_t)


def candidates(n, d, m):
    return np.random.RandomState(300 + n + d + m).uniform(size=(m, d))


def grad_points(n, d):
    """GRAD_B points: uniform ones, one ON an observation (the smallest sd), two a step off
    one, the corners, and one far outside the unit cube (k* underflows: the prior)."""
    X = inputs(n, d)[0]
    rng = np.random.RandomState(400 + n + d)
    P = np.vstack([rng.uniform(size=(GRAD_B - 6, d)), X[0], X[0] + 1e-3, X[n // 2] - 2e-3, np.zeros(d), np.ones(d),
                   np.full(d, 60.0)])
    assert P.shape == (GRAD_B, d)
    return P


def _split(a):
    """An ``np.longdouble`` array as (hi, lo) fp64 halves."""
    a = np.asarray(a, dtype=np.longdouble)
    hi = a.astype(np.float64)
    return hi, (a - hi).astype(np.float64)


def join(hi, lo):
    return hi.astype(np.longdouble) + lo.astype(np.longdouble)


def make():
    """Compute every reference and check the fixtures' top-k gaps; returns the arrays to store."""
    out = {}
    for n, d, m in SCORE:
        fm, tm = pair(n, d)
        C, y_opt = candidates(n, d, m), inputs(n, d)[5]
        for acq in ACQS:
            v80, V = R.values(fm, tm, C, y_opt, acq, XI, "exact")
            v64, _ = R.values(fm, tm, C, y_opt, acq, XI, "fp64")
            assert np.all(V > 0) and np.all(np.isfinite(V)), (n, d, m, acq)
            k = min(TOPK, m)
            assert R.gaps_hold(v80.astype(np.float64), k), f"top-k gaps fail: {(n, d, m, acq)}"
            key = f"score_{n}_{d}_{m}_{acq}"
            out[key + "_hi"], out[key + "_lo"] = _split(v80)
            out[key + "_scale"] = V
            out[key + "_err64"] = np.abs(v64.astype(np.longdouble) - v80).astype(np.float64) / V
            out[key + "_top"] = R.topk(v80.astype(np.float64), k)
            print(key, "fp64 error / scale", out[key + "_err64"].max(), flush=True)
    for n, d in GRAD:
        fm, tm = pair(n, d)
        P, y_opt = grad_points(n, d), inputs(n, d)[5]
        for acq in ACQS:
            rows = [(R.value_grad(fm, tm, x, y_opt, acq, XI, "exact"), R.value_grad(fm, tm, x, y_opt, acq, XI, "fp64"))
                    for x in P]
            key = f"grad_{n}_{d}_{acq}"
            out[key + "_f_hi"], out[key + "_f_lo"] = _split([r[0][0] for r in rows])
            out[key + "_g_hi"], out[key + "_g_lo"] = _split([r[0][1] for r in rows])
            out[key + "_parts"] = np.array([[float(p) for p in r[0][4]] for r in rows])
            V = np.array([r[0][2] for r in rows])
            G = np.array([r[0][3] for r in rows])
            out[key + "_f_scale"], out[key + "_g_scale"] = V, G
            ef = np.array([abs(np.longdouble(r[1][0]) - r[0][0]) for r in rows], dtype=np.float64)
            eg = np.array([np.abs(r[1][1].astype(np.longdouble) - r[0][1]) for r in rows], dtype=np.float64)
            out[key + "_f_err64"] = np.where(V > 0, ef / np.where(V > 0, V, 1.0), np.where(ef == 0, 0.0, np.inf))
            out[key + "_g_err64"] = np.where(G > 0, eg / np.where(G > 0, G, 1.0), np.where(eg == 0, 0.0, np.inf))
            print(key, "fp64 error / scale: f", out[key + "_f_err64"].max(), "g", out[key + "_g_err64"].max(), flush=True)
    return out


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


# ---- sd = 0, decided by the inputs -------------------------------------------------------------
#: (n, d): one observation; a few; more than the 16 waves' rows; more observations than one wave;
#: the first n on the 4-wave polish kernel (fp64 reference only, 8 + 8 points)
SD0 = [(1, 1), (6, 3), (17, 5), (65, 4), (915, 5)]
#: the negative models' length scale, the same in every dimension.  At n = 915 the closest pair
#: of the observations is 0.026 apart and K - amp / 2 I is not positive definite at ls = 0.05
#: (smallest eigenvalue -0.32 amp; -0.005 amp at 0.025): 0.02 leaves 0.129 amp
SD0_LS = {None: 0.05, 915: 0.02}
SD0_STEP = 0.2
SD0_UNIFORM = 16
#: the uniform points' seed where 500 + n + d does not serve: in one dimension a draw within
#: 0.027 of the single observation has a variance between the two margins (neither "on" nor
#: "off"; 16 draws miss that window with probability 0.4) and the guard would fail
SD0_USEED = {(1, 1): 806}
SD0_LARGE_POINTS = 8          # "on" and "off" points each at n past the 80-bit factor
SD0_EXACT_MAX_N = 600
#: the guard's margins: the normalised variance at an "on" point is <= -0.1 amp (the exact value
#: is -1.0 amp up to the neighbours' kernel values), at an "off" point >= 1e-6 amp (the rule of
#: tests/factor_cases.py for its own points)
SD0_ON_MAX, SD0_OFF_MIN = -0.1, 1e-6
#: (name, objective model negative, log-time model negative)
SD0_PAIRINGS = [("both", True, True), ("f_only", True, False), ("t_only", False, True), ("neither", False, False)]


@functools.lru_cache(maxsize=None)
def sd0_inputs(n, d):
    """``(X, y, logt, neg_f, neg_t, pos_f, pos_t, P, on, y_opt)``: the observations (uniform in
    the unit cube) and targets of ``inputs(n, d)`` under two sets of models.  ``neg_f`` = (amp
    1.3, ls ``SD0_LS`` in every dimension, noise -amp / 2) and ``neg_t`` = (amp 0.8, the same
    ls, noise -0.4).  With A = K + noise I = K - amp
    / 2 I positive definite, the posterior variance at observation i is ``amp - (A + amp / 2
    I)_i A^-1 (A + amp / 2 I)_i = amp - (A + amp I + amp^2 / 4 A^-1)_ii <= amp - (amp / 2 + amp
    + amp / 2) = -amp``, because ``(A^-1)_ii >= 1 / A_ii``: every precision clamps it to sd = 0.
    ``pos_f`` / ``pos_t`` are the positive-noise thetas of ``inputs(n, d)``.  The points ``P``:
    every observation itself (``on`` True), every observation shifted by 0.2 in every
    coordinate and clipped to the cube, then 16 uniform points (``on`` False; the
    variance is 0.27 .. 1.0 amp there under the negative models).  Past ``SD0_EXACT_MAX_N`` observations: 8 "on" and 8 "off"
    points (4 shifted, 4 uniform)."""
    X, y, logt, pos_f, pos_t, y_opt = inputs(n, d)
    ls = np.full(d, SD0_LS.get(n, SD0_LS[None]))
    U = np.random.RandomState(SD0_USEED.get((n, d), 500 + n + d)).uniform(size=(SD0_UNIFORM, d))
    shifted = np.clip(X + SD0_STEP, 0.0, 1.0)
    if n > SD0_EXACT_MAX_N:
        h = SD0_LARGE_POINTS
        P = np.vstack([X[:h], shifted[:h // 2], U[:h - h // 2]])
        on = np.arange(len(P)) < h
    else:
        P = np.vstack([X, shifted, U])
        on = np.arange(len(P)) < n
    for a in (ls, P, on):
        a.setflags(write=False)
    return X, y, logt, (1.3, ls, -1.3 / 2), (0.8, ls, -0.4), pos_f, pos_t, P, on, y_opt


@functools.lru_cache(maxsize=None)
def sd0_models(n, d):
    """``{"neg_f", "neg_t", "pos_f", "pos_t"}`` -> the reference model (shared, factors lazy)."""
    X, y, logt, neg_f, neg_t, pos_f, pos_t = sd0_inputs(n, d)[:7]
    return {"neg_f": R.Model(X, y, *neg_f), "neg_t": R.Model(X, logt, *neg_t),
            "pos_f": R.Model(X, y, *pos_f), "pos_t": R.Model(X, logt, *pos_t)}


def sd0_pair(n, d, pairing):
    """The reference ``(f, tau)`` models of a pairing name of ``SD0_PAIRINGS``."""
    _, nf, nt = next(p for p in SD0_PAIRINGS if p[0] == pairing)
    mdl = sd0_models(n, d)
    return mdl["neg_f" if nf else "pos_f"], mdl["neg_t" if nt else "pos_t"]


def normalised_variance(mdl, P, precision):
    """``amp - |W k*|^2`` at the rows of P, NOT clamped, over amp: "exact" in ``np.longdouble``
    on the 80-bit factor, "fp64" on scipy's."""
    st = mdl.st
    if precision == "exact":
        Kx, W = O.matern52_exact(P, st.X, st.length_scale, st.amp), mdl.exact[1]
        amp = np.longdouble(st.amp)
    else:
        Kx, W, amp = O.matern52(P, st.X, st.length_scale, st.amp), mdl.w64, st.amp
    V = Kx @ W.T
    return ((amp - (V * V).sum(1)) / amp).astype(np.float64)


# ---- the search's own y_opt, and lower ---------------------------------------------------------
GOLDEN_EDGES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "acq_ps_edges_ref.npz")
#: the scoring pairs and gradient tables that run again at the search's y_opt and below it
EDGE_SCORE = [SCORE[1], SCORE[2]]
EDGE_GRAD = [GRAD[1], GRAD[2]]
EDGE_MODES = ("min", "low")
#: classes by the reference z = (y_opt - xi - mu) / sd: below Z_DEAD the normal cdf and pdf are
#: exactly 0 in fp64 with a margin (the cdf's last subnormal is at z = -38.5, the pdf's at -38.6),
#: above Z_LIVE both are normal numbers (cdf(-37) = 6e-300)
Z_DEAD, Z_LIVE = -40.0, -37.0
DEAD, BAND, LIVE = 0, 1, 2
EDGE_SCORE_C = 16             # y_opt = min(y) - c std(y): the smallest power of two that leaves a
EDGE_SHARE = 0.25             # quarter of every scoring case dead and a quarter live (asserted)
EDGE_GRAD_DEAD_MIN = 3        # gradient tables: the smallest c with this many of the 15 points dead


def edge_y_opt(n, d, mode, c=None):
    y = inputs(n, d)[1]
    if mode == "min":
        return float(np.min(y))
    return float(np.min(y) - c * np.std(y))


def z_exact(fm, P, y_opt, precision="exact"):
    """The reference z at the rows of P under the objective's model (fp64 values of the
    precision's arithmetic; -inf where sd = 0)."""
    rows = [fm.posterior_grad(x, precision)[:2] for x in P]
    t = LD if precision == "exact" else np.float64
    return np.array([float((t(y_opt) - t(XI) - t(mu)) / t(sd)) if sd > 0 else -np.inf for mu, sd in rows])


def classify(z):
    return np.where(z < Z_DEAD, DEAD, np.where(z > Z_LIVE, LIVE, BAND)).astype(np.int8)


def band_bound(fm, tm, P, y_opt, acq, precision="exact"):
    """What |v| cannot exceed at a point whose z is <= Z_LIVE: EI = sd (z cdf(z) + pdf(z)) and
    PI = cdf(z) grow with z, so |v| <= (sd (Z_LIVE cdf(Z_LIVE) + pdf(Z_LIVE)) or cdf(Z_LIVE))
    inv_t; times 1 + 1e-6 for the rounding of sd, inv_t and of the device's cdf / pdf (a few ulp
    each).  Band points are held to this only: between z = -40 and -37 cdf and pdf pass through
    the subnormals, where a relative bar against another library's values means nothing."""
    from scipy.stats import norm

    out = []
    for x in P:
        sd = float(fm.posterior_grad(x, precision)[1])
        mt, s = (float(v) for v in tm.posterior_grad(x, precision)[:2])
        a = sd * (Z_LIVE * norm.cdf(Z_LIVE) + norm.pdf(Z_LIVE)) if acq == "EI" else norm.cdf(Z_LIVE)
        out.append(a * np.exp(-mt + s * s / 2) * (1 + 1e-6))
    return np.array(out)


def grad_c(n, d):
    """The smallest power of two c for which ``EDGE_GRAD_DEAD_MIN`` of the gradient points are dead."""
    fm = pair(n, d)[0]
    c = 1
    while np.sum(classify(z_exact(fm, grad_points(n, d), edge_y_opt(n, d, "low", c))) == DEAD) < EDGE_GRAD_DEAD_MIN:
        c *= 2
        assert c <= 2 ** 20, (n, d)
    return c


def make_edges():
    """The references at ``min(y)`` and below it, with the classes, shares and top-k gaps
    asserted here, where the fixture is made: nothing is excused at run time."""
    out = {}
    for n, d, m in EDGE_SCORE:
        fm, tm = pair(n, d)
        C = candidates(n, d, m)
        for mode in EDGE_MODES:
            y_opt = edge_y_opt(n, d, mode, EDGE_SCORE_C)
            z = z_exact(fm, C, y_opt)
            cls = classify(z)
            shares = [int(np.sum(cls == k)) for k in (DEAD, BAND, LIVE)]
            print(f"edges score ({n}, {d}, {m}) y_opt={mode}: dead / band / live = {shares}, z in "
                  f"[{z.min():.1f}, {z.max():.1f}]", flush=True)
            if mode == "low":
                assert shares[0] >= EDGE_SHARE * m and shares[2] >= EDGE_SHARE * m, (n, d, m, shares)
                half = classify(z_exact(fm, C, edge_y_opt(n, d, "low", EDGE_SCORE_C // 2)))
                assert np.sum(half == DEAD) < EDGE_SHARE * m or np.sum(half == LIVE) < EDGE_SHARE * m, \
                    f"c = {EDGE_SCORE_C // 2} meets the shares already: {(n, d, m)}"
            key = f"score_{n}_{d}_{m}_{mode}"
            out[key + "_z"], out[key + "_cls"], out[key + "_yopt"] = z, cls, np.float64(y_opt)
            for acq in ACQS:
                v80, V = R.values(fm, tm, C, y_opt, acq, XI, "exact")
                v64, _ = R.values(fm, tm, C, y_opt, acq, XI, "fp64")
                live = cls == LIVE
                assert np.all(v80[cls == DEAD] == 0) and np.all(V[cls == DEAD] == 0), (key, acq)
                assert np.all(V[live] > 0) and np.all(v80[live] < 0), (key, acq)
                k = min(TOPK, int(live.sum()))
                lv = np.where(live, v80.astype(np.float64), np.inf)
                assert R.gaps_hold(lv, k), f"top-k gaps of the live values fail: {(key, acq)}"
                bound = band_bound(fm, tm, C, y_opt, acq)
                assert np.all(np.abs(v80[cls != LIVE].astype(np.float64)) <= bound[cls != LIVE]), (key, acq)
                assert np.all(-lv[R.topk(lv, k)] > bound.max()), f"a top-k value is inside the band's bound: {(key, acq)}"
                out[f"{key}_{acq}_hi"], out[f"{key}_{acq}_lo"] = _split(v80)
                out[f"{key}_{acq}_scale"] = V
                e = np.abs(v64.astype(np.longdouble) - v80).astype(np.float64)
                out[f"{key}_{acq}_err64"] = np.where(live, e / np.where(V > 0, V, 1.0), 0.0)
                out[f"{key}_{acq}_top"] = R.topk(lv, k)
                out[f"{key}_{acq}_band"] = bound
                print(f"  {acq}: fp64 error / scale on the live points {out[f'{key}_{acq}_err64'].max():.3e}", flush=True)
    for n, d in EDGE_GRAD:
        fm, tm = pair(n, d)
        P = grad_points(n, d)
        c = grad_c(n, d)
        for mode in EDGE_MODES:
            y_opt = edge_y_opt(n, d, mode, c)
            z = z_exact(fm, P, y_opt)
            cls = classify(z)
            print(f"edges grad ({n}, {d}) y_opt={mode} (c = {c}): dead / band / live = "
                  f"{[int(np.sum(cls == k)) for k in (DEAD, BAND, LIVE)]}", flush=True)
            if mode == "low":
                assert np.sum(cls == DEAD) >= EDGE_GRAD_DEAD_MIN
            key = f"grad_{n}_{d}_{mode}"
            out[key + "_z"], out[key + "_cls"], out[key + "_yopt"], out[key + "_c"] = z, cls, np.float64(y_opt), np.int64(c)
            for acq in ACQS:
                rows = [(R.value_grad(fm, tm, x, y_opt, acq, XI, "exact"), R.value_grad(fm, tm, x, y_opt, acq, XI, "fp64"))
                        for x in P]
                dead = cls == DEAD
                assert all(r[0][0] == 0 and np.all(r[0][1] == 0) for r, dd in zip(rows, dead) if dd), (key, acq)
                k2 = f"{key}_{acq}"
                out[k2 + "_f_hi"], out[k2 + "_f_lo"] = _split([r[0][0] for r in rows])
                out[k2 + "_g_hi"], out[k2 + "_g_lo"] = _split([r[0][1] for r in rows])
                V = np.array([r[0][2] for r in rows])
                G = np.array([r[0][3] for r in rows])
                out[k2 + "_f_scale"], out[k2 + "_g_scale"] = V, G
                ef = np.array([abs(np.longdouble(r[1][0]) - r[0][0]) for r in rows], dtype=np.float64)
                eg = np.array([np.abs(r[1][1].astype(np.longdouble) - r[0][1]) for r in rows], dtype=np.float64)
                out[k2 + "_f_err64"] = np.where(V > 0, ef / np.where(V > 0, V, 1.0), np.where(ef == 0, 0.0, np.inf))
                out[k2 + "_g_err64"] = np.where(G > 0, eg / np.where(G > 0, G, 1.0), np.where(eg == 0, 0.0, np.inf))
                out[k2 + "_band"] = band_bound(fm, tm, P, y_opt, acq)
    return out


@functools.lru_cache(maxsize=None)
def golden_edges():
    with np.load(GOLDEN_EDGES) as z:
        return {k: z[k] for k in z.files}


if __name__ == "__main__":
    import sys

    if sys.argv[1:] == ["edges"]:
        np.savez_compressed(GOLDEN_EDGES, **make_edges())
        print("wrote", GOLDEN_EDGES, os.path.getsize(GOLDEN_EDGES), "bytes")
    else:
        np.savez_compressed(GOLDEN, **make())
        print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
