"""The CPU guard of the acquisition edge fixtures (no GPU): the ``sd = 0`` models of
``ps_cases.sd0_inputs`` -- both factorizations succeed and every point is on the side of zero
the fixture says, with a margin, in fp64 and (where it runs) in 80 bits -- and the stored
classes, shares and references of the runs at the search's own ``y_opt`` and below it
(tests/golden/acq_ps_edges_ref.npz).  No point is ever dropped: a point between the margins
fails the guard."""
import numpy as np
import pytest

from tests import ps_cases as C
from tests import ps_ref as R


@pytest.mark.parametrize("n,d", C.SD0, ids=lambda v: str(v))
def test_sd0_points_are_on_their_side_of_zero(n, d):
    X, y, logt, neg_f, neg_t, pos_f, pos_t, P, on, y_opt = C.sd0_inputs(n, d)
    assert neg_f[2] == -neg_f[0] / 2 and neg_t[2] == -neg_t[0] / 2 == -0.4
    if n <= C.SD0_EXACT_MAX_N:
        assert len(P) == 2 * n + C.SD0_UNIFORM and on.sum() == n and np.all(P[:n] == X)
        assert np.all(P[n:2 * n] == np.clip(X + C.SD0_STEP, 0.0, 1.0))
    else:
        assert on.sum() == C.SD0_LARGE_POINTS == (~on).sum()
    assert np.all((P >= 0) & (P <= 1))
    # both kinds inside one 64-lane wave of the scoring pass (and inside the one polish batch)
    assert any(on[w:w + 64].any() and (~on[w:w + 64]).any() for w in range(0, len(P), 64))
    mdl = C.sd0_models(n, d)          # gp_from_theta raises LinAlgError on a failed pivot
    for name in ("neg_f", "neg_t"):
        m = mdl[name]
        precisions = ["fp64"] + (["exact"] if n <= C.SD0_EXACT_MAX_N else [])
        for precision in precisions:
            if precision == "exact":
                m.exact               # the 80-bit factor: raises on a failed pivot
            var = C.normalised_variance(m, P, precision)
            print(f"sd0 ({n}, {d}) {name} {precision}: var / amp on [{var[on].min():.6f}, {var[on].max():.6f}], "
                  f"off [{var[~on].min():.6f}, {var[~on].max():.6f}]")
            assert np.all(var[on] <= C.SD0_ON_MAX), (name, precision, float(var[on].max()))
            assert np.all(var[~on] >= C.SD0_OFF_MIN), (name, precision, float(var[~on].min()))
        # the reference's own sd: exactly 0 on, positive off
        sd = np.array([float(m.posterior_grad(x, "fp64")[1]) for x in P])
        assert np.all(sd[on] == 0.0) and np.all(sd[~on] > 0)
    for name in ("pos_f", "pos_t"):
        var = C.normalised_variance(mdl[name], P, "fp64")
        print(f"sd0 ({n}, {d}) {name} fp64: var / amp on [{var[on].min():.3e}, {var[on].max():.3e}], off min "
              f"{var[~on].min():.3e}")
        assert np.all(var >= 1e-3)    # the positive-noise models: sd > 0 everywhere (noise / (amp + noise) at least)


def test_sd0_reference_answers_zero_at_on_points():
    """``ps_ref.value_grad`` at an "on" point: a = 0, v = 0, g = 0 with ``sd_f = 0``; with ``sd_t
    = 0`` only, inv_t = exp(-mu_t) and the value is live."""
    n, d = 6, 3
    P, on = C.sd0_inputs(n, d)[7:9]
    y_opt = C.sd0_inputs(n, d)[9]
    for pairing, nf, nt in C.SD0_PAIRINGS:
        fm, tm = C.sd0_pair(n, d, pairing)
        for acq in C.ACQS:
            for x in P[on]:
                v, g, V, G, parts = R.value_grad(fm, tm, x, y_opt, acq, C.XI, "exact")
                if nf:
                    assert v == 0 and np.all(g == 0) and parts[0] == 0 and V == 0
                else:
                    assert v < 0 and V > 0
                if nt:
                    assert parts[3] == 0 and parts[1] == np.exp(-parts[2])
                else:
                    assert parts[3] > 0


# ---- the search's own y_opt, and lower ----------------------------------------------------------
def test_edge_classes_and_shares():
    g = C.golden_edges()
    for n, d, m in C.EDGE_SCORE:
        y = C.inputs(n, d)[1]
        for mode in C.EDGE_MODES:
            key = f"score_{n}_{d}_{m}_{mode}"
            cls, z = g[key + "_cls"], g[key + "_z"]
            assert float(g[key + "_yopt"]) == C.edge_y_opt(n, d, mode, C.EDGE_SCORE_C)
            assert np.all(cls == C.classify(z)) and len(cls) == m
            dead, band, live = (int(np.sum(cls == k)) for k in (C.DEAD, C.BAND, C.LIVE))
            print(f"edges ({n}, {d}, {m}) y_opt = {mode}: dead {dead} / band {band} / live {live} of {m}; "
                  f"z in [{z.min():.1f}, {z.max():.1f}]")
            if mode == "low":
                assert dead >= C.EDGE_SHARE * m and live >= C.EDGE_SHARE * m
            else:
                # the finding: at the search's own y_opt nothing underflows in these fixtures
                assert float(g[key + "_yopt"]) == float(np.min(y))
            for acq in C.ACQS:
                v = C.join(g[f"{key}_{acq}_hi"], g[f"{key}_{acq}_lo"])
                V = g[f"{key}_{acq}_scale"]
                assert np.all(v[cls == C.DEAD] == 0) and np.all(V[cls == C.DEAD] == 0)
                assert np.all(v[cls == C.LIVE] < 0) and np.all(V[cls == C.LIVE] > 0)
                assert np.all(np.abs(v[cls != C.LIVE]).astype(np.float64) <= g[f"{key}_{acq}_band"][cls != C.LIVE])
                lv = np.where(cls == C.LIVE, v.astype(np.float64), np.inf)
                assert R.gaps_hold(lv, C.TOPK) and list(g[f"{key}_{acq}_top"]) == list(R.topk(lv, C.TOPK))
    # the stated shares of the two lowered cases
    assert [int(np.sum(g["score_17_3_65_low_cls"] == k)) for k in (0, 1, 2)] == [40, 6, 19]
    assert [int(np.sum(g["score_40_5_257_low_cls"] == k)) for k in (0, 1, 2)] == [107, 32, 118]
    for n, d in C.EDGE_GRAD:
        cls = g[f"grad_{n}_{d}_low_cls"]
        c = int(g[f"grad_{n}_{d}_low_c"])
        print(f"edges grad ({n}, {d}): c = {c}, dead {int(np.sum(cls == C.DEAD))} of {len(cls)}")
        assert np.sum(cls == C.DEAD) >= C.EDGE_GRAD_DEAD_MIN and c & (c - 1) == 0
        for acq in C.ACQS:
            k2 = f"grad_{n}_{d}_low_{acq}"
            dead = cls == C.DEAD
            assert np.all(g[k2 + "_f_hi"][dead] == 0) and np.all(g[k2 + "_g_hi"][dead] == 0)
            assert np.all(g[k2 + "_f_scale"][dead] == 0) and np.all(g[k2 + "_g_scale"][dead] == 0)


def test_edge_golden_is_current_and_c_is_the_smallest():
    """The committed edge references are those of the fixtures as they stand (the small scoring
    pair and gradient table, recomputed), c = 16 is the smallest power of two that meets the
    shares, and the file is no larger than the main golden file."""
    import os

    g = C.golden_edges()
    n, d, m = C.EDGE_SCORE[0]
    fm, tm = C.pair(n, d)
    cand = C.candidates(n, d, m)
    for mode in C.EDGE_MODES:
        y_opt = C.edge_y_opt(n, d, mode, C.EDGE_SCORE_C)
        key = f"score_{n}_{d}_{m}_{mode}"
        z = C.z_exact(fm, cand, y_opt)
        assert np.all(z == g[key + "_z"])
        for acq in C.ACQS:
            v, V = R.values(fm, tm, cand, y_opt, acq, C.XI, "exact")
            live = g[key + "_cls"] == C.LIVE       # the (hi, lo) split is exact only away from the subnormals
            assert np.all(C.join(g[f"{key}_{acq}_hi"], g[f"{key}_{acq}_lo"])[live] == v[live])
            assert np.all(g[f"{key}_{acq}_scale"] == V)
            assert np.all(g[f"{key}_{acq}_band"] == C.band_bound(fm, tm, cand, y_opt, acq))
    oks = []
    for n2, d2, m2 in C.EDGE_SCORE:
        half = C.classify(C.z_exact(C.pair(n2, d2)[0], C.candidates(n2, d2, m2),
                                    C.edge_y_opt(n2, d2, "low", C.EDGE_SCORE_C // 2)))
        oks.append(np.sum(half == C.DEAD) >= C.EDGE_SHARE * m2 and np.sum(half == C.LIVE) >= C.EDGE_SHARE * m2)
        print(f"c = {C.EDGE_SCORE_C // 2} at ({n2}, {d2}, {m2}): dead {int(np.sum(half == C.DEAD))}, live "
              f"{int(np.sum(half == C.LIVE))} of {m2}")
    assert not all(oks), "half the c meets the shares in every case"
    n, d = C.EDGE_GRAD[0]
    assert C.grad_c(n, d) == int(g[f"grad_{n}_{d}_low_c"])
    x = C.grad_points(n, d)[3]
    y_opt = float(g[f"grad_{n}_{d}_low_yopt"])
    one = R.value_grad(*C.pair(n, d), x, y_opt, "EI", C.XI, "exact")
    assert C.join(g[f"grad_{n}_{d}_low_EI_f_hi"], g[f"grad_{n}_{d}_low_EI_f_lo"])[3] == one[0]
    assert os.path.getsize(C.GOLDEN_EDGES) <= os.path.getsize(C.GOLDEN)
