"""CPU checks of the refit objective's case table (``tests/lml_cases.py``): the table
reaches every kernel path of ``csrc/gp_fit.hip``, and the fp64 oracle the device is
compared with sits far inside the device's bar."""
import os
import re

import numpy as np
import pytest

from tests import lml_cases as C
from tests.conftest import ROOT

EPS = np.finfo(float).eps


def test_table_reaches_every_kernel_and_instantiation():
    """Every (kernel, dp) that exists has a case.  A changed threshold (in gp_fit.hip
    and the restated rule) that takes a combination's last case away fails here by name."""
    reached = {}
    for c in C.CASES:
        kernel, dp, _ = C.path(*c)
        reached.setdefault((kernel, dp), []).append(C.case_id(c))
    lost = [f"{k} x dp={dp}" for k, dp in C.COMBINATIONS if (k, dp) not in reached]
    assert not lost, f"no case reaches: {lost}"
    assert set(reached) == set(C.COMBINATIONS), set(reached) - set(C.COMBINATIONS)


def test_rule_at_the_structural_edges():
    """The restated rule at the edges the table is built on, spelled out."""
    assert [C.fit_dp(d) for d in (1, 4, 5, 8, 9, 12, 13, 16, 17, 32, 33)] == [4, 4, 8, 8, 12, 12, 16, 16, 32, 32, -1]
    assert C.path(48, 32)[0] == "panel" and C.path(49, 16)[0] == "split-fused"
    assert C.path(200, 17, "panel")[0] == "panel" and C.path(201, 17, "panel")[0] == "split-fused"
    assert C.path(16, 32, "split")[0] == "panel" and C.path(17, 32, "split") == ("split-fused", 32, True)
    # the fused limits, and the first n past each
    for n, d, dp in [(256, 17, 32), (512, 13, 16), (672, 9, 12), (1024, 5, 8)]:
        assert C.path(n, d) == ("split-fused", dp, True)
        assert C.path(n + 1, d) == ("split-unfused", dp, False)
    assert C.path(2048, 4) == ("split-fused", 4, True)
    with pytest.raises(ValueError):
        C.path(2049, 4)
    # every shape of the unfused rows is the smallest n of its dp there
    for c in C.SPLIT_UNFUSED:
        assert C.path(c.n - 1, c.d)[0] == "split-fused"


def test_rule_constants_are_the_kernels():
    """The thresholds restated in lml_cases.py are the ones gp_fit.hip compiles."""
    src = open(os.path.join(ROOT, "mpi_opt_amd", "csrc", "gp_fit.hip")).read()
    hdr = open(os.path.join(ROOT, "mpi_opt_amd", "csrc", "mpo_internal.h")).read()

    def const(name, text=src):
        m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", text)
        assert m, name
        return int(m.group(1))

    assert const("kSwNb") == C.K_SW_NB
    assert const("kSplitMinN") == C.K_SPLIT_MIN_N
    assert const("kFitLdsMaxN") == C.K_FIT_LDS_MAX_N
    assert const("kMaxGroup") == C.K_MAX_GROUP
    assert const("kMaxObs", hdr) == C.K_MAX_OBS
    assert "xs_lds <= 64 * 1024" in src and 64 * 1024 // 8 == C.K_FUSED_DOUBLES


@pytest.mark.parametrize("case", [c for c in C.CASES if c.n <= 513], ids=C.case_id)
def test_oracle_lml_within_one_unit_of_longdouble(case):
    """``oracle.gp_ei.lml_and_grad``'s LML against an 80-bit Cholesky LML of the same
    K: at most 1 unit of cond(K) * eps * max(1, |lml|).

    Measured on these inputs.  On the panel cases (device bar 50 units): 0.63 and 0.41
    units at n = 1, where cond(K) = 1 and the unit is one rounding of the result itself;
    0.21 at n = 2; at most 0.09 from n = 7 on.  On the sweep's cases (device bar 1000
    units): 0.12 at (17, 32), at most 0.033 from n = 49 on, at most 0.0062 from n = 256
    on.  Past n = 513 the 80-bit factorisation takes seconds per theta (10 s at
    n = 2048), so it was run once and is not part of the suite: 0.0010 and 0.0010 units
    at (672, 12), 0.0007 and 0.0011 at (673, 9), 0.0041 and 0.0009 at (1024, 8), 0.0060
    and 0.0018 at (1025, 5), 0.0026 and 0.0013 at (2048, 4), for noise 1e-2 and 0.2.
    The oracle therefore sits a factor of 80 inside the panel bar where the unit is a
    single rounding, and 10^4 or more inside the sweep's bar from n = 49 on."""
    X, yn, T, lml, _ = C.reference(case.n, case.d)
    for t, v in zip(T, lml):
        K = C.gram(X, t)
        ref = C.lml_longdouble(K, yn)
        unit = np.linalg.cond(K) * EPS * max(1.0, abs(float(ref)))
        err = abs(float(np.longdouble(v) - ref))
        print(f"{C.case_id(case)} noise {np.exp(t[-1]):g}: {err / unit:.2e} units of cond*eps")
        assert err <= unit, (err, unit)
