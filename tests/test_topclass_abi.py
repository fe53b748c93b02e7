"""Host side of the topclass C ABI (mpo_tc_*, csrc/topclass.hip): plan building and
validation need no GPU.  Also the coverage of the GPU tests' case table
(tests/topclass_cases.py), which the issue prescribes."""
import ctypes

import numpy as np
import pytest

from mpi_opt_amd import _lib
from mpi_opt_amd.topclass import PARAM_NAMES, TopclassSpec
from tests import topclass_cases as TC

MPO_EINVAL, MPO_ENOTSUP = 1, 3


def create(members, batch=4, H=150, W=94, C=5, classes=3):
    """members: (kernel_size, lr, dropout, seed, options) -> (status, handle, message)."""
    L = _lib.lib()
    arr = (_lib.MpoTcSpec * len(members))(*[_lib.MpoTcSpec(*m) for m in members])
    h = ctypes.c_void_p()
    rc = L.mpo_tc_create(arr, len(members), batch, H, W, C, classes, ctypes.byref(h))
    return rc, h, (L.mpo_last_error() or b"").decode()


OK = (3, 1e-3, 0.5, 0, 0)


@pytest.mark.parametrize("kw,word", [
    (dict(members=[(0, 1e-3, 0.5, 0, 0)]), "kernel_size 0"),
    (dict(members=[OK, (10, 1e-3, 0.5, 0, 0)]), "member 1 has kernel_size 10"),
    (dict(members=[OK], C=9), "C 1..8"),
    (dict(members=[OK], H=17), "conv2 output of 1 x"),            # (17 - 3) // 3 + 1 = 5, (5 - 3) // 3 + 1 = 1
    (dict(members=[(9, 1e-3, 0.5, 0, 0)], H=150, W=41), "conv2 output of"),
    (dict(members=[OK], classes=1), "classes"),
    (dict(members=[OK], classes=17), "classes"),
    (dict(members=[(3, 1e-3, 0.5, 0, 0x2)]), "options 0x2"),
    (dict(members=[(3, 1e-3, 0.5, 0, 0x200)]), "options 0x200"),
    (dict(members=[(3, 0.0, 0.5, 0, 0)]), "lr"),
    (dict(members=[(3, 1e-3, float("nan"), 0, 0)]), "dropout"),
    (dict(members=[OK], H=257), "H, W 1..256"),
])
def test_create_refuses_with_a_message(kw, word):
    rc, h, msg = create(**kw)
    assert rc == MPO_ENOTSUP and not h.value and word in msg, (rc, msg)


def test_create_argument_errors():
    rc, h, msg = create([OK], batch=0)
    assert rc == MPO_EINVAL and "batch" in msg
    rc, h, msg = create([OK], batch=257)
    assert rc == MPO_EINVAL
    L = _lib.lib()
    assert L.mpo_tc_create(None, 1, 4, 150, 94, 5, 3, ctypes.byref(ctypes.c_void_p())) == MPO_EINVAL
    assert L.mpo_tc_sizes(None, None) == MPO_EINVAL


def test_layouts_are_contiguous_and_match_param_shapes():
    L = _lib.lib()
    ks = [1, 3, 6, 9]
    rc, h, msg = create([(k, 1e-3, 0.5, i, 0x101) for i, k in enumerate(ks)], batch=7, classes=5)
    assert rc == 0, msg
    sz = _lib.MpoPopSizes()
    assert L.mpo_tc_sizes(h, ctypes.byref(sz)) == 0 and (sz.n_members, sz.batch) == (4, 7)
    offs = (ctypes.c_int64 * 9)()
    end = 0
    for i, k in enumerate(ks):
        assert L.mpo_tc_param_layout(h, i, offs) == 0
        o = [int(v) for v in offs]
        shapes = TopclassSpec(kernel_size=k, classes=5).param_shapes()
        assert o[0] == end                                       # members follow each other
        for j, n in enumerate(PARAM_NAMES):
            cnt = int(np.prod(shapes[n]))
            assert o[j] % 64 == 0 and o[j] + cnt <= o[j + 1] < o[j] + cnt + 64, (i, n)   # contiguous, 64-float aligned
        end = o[8]
    assert end == sz.n_params and sz.act_floats > 0 and sz.table_bytes > 0
    assert L.mpo_tc_param_layout(h, 4, offs) == MPO_EINVAL
    aoffs = (ctypes.c_int64 * 12)()
    assert L.mpo_tc_act_layout(h, 0, aoffs) == 0 and list(aoffs) == sorted(aoffs) and aoffs[11] < sz.act_floats
    # unbound handles refuse to step
    assert L.mpo_tc_train_step(h, 1, 1, 1, 7, 0, 0, 1, None) == MPO_EINVAL
    assert b"mpo_tc_bind" in L.mpo_last_error()
    assert L.mpo_tc_destroy(h) == 0


def test_python_specs_refuse_what_the_abi_refuses():
    for kw in (dict(kernel_size=0), dict(kernel_size=10), dict(input_shape=(150, 94, 9)), dict(input_shape=(17, 94, 5)),
               dict(classes=1), dict(input_shape=(300, 94, 5))):
        with pytest.raises(ValueError):
            TopclassSpec(**kw).geometry()


def test_case_table_covers_what_the_issue_lists():
    cases = TC.CASES
    smallest = {c.members[0][0]: c for c in cases if c.name.endswith("_smallest")}
    assert sorted(smallest) == list(range(1, 10))
    for k, c in smallest.items():
        assert c.shape[:2] == (4 * k + 6, 4 * k + 6)
        with pytest.raises(ValueError):                          # one less is illegal
            TopclassSpec(kernel_size=k, input_shape=(4 * k + 5, 4 * k + 6, c.shape[2])).geometry()
    res = [r for c in cases for r in TC.residues(c)]
    for key in ("c1h", "c1w", "c2h", "c2w"):
        assert {1, 2} <= {r[key] for r in res}, key
    assert {r["H2"] % 2 for r in res} == {0, 1} and {r["W2"] % 2 for r in res} == {0, 1}
    assert {c.shape[2] for c in cases} >= {1, 5} and smallest[1].shape[2] == 5
    assert {c.classes for c in cases} == {3, 5} and {c.batch for c in cases} >= {1, 3, 7}
    assert {m[1] for c in cases for m in c.members} >= {0.0, 0.3, 1.0}
    assert any(len({m[0] for m in c.members}) > 1 for c in cases)
    ref = [c for c in cases if c.shape == (150, 94, 5)]
    assert len(ref) == 1 and [m[0] for m in ref[0].members] == [1, 3, 6] and ref[0].batch == 4
    assert sorted(m[0] for m in TC.SECOND_STEP.members) == [1, 5]
    assert {(m[3], m[2]) for m in TC.TRAJECTORY.members} == {("adam", TC.BCE), ("adam", TC.CCE), ("sgd", TC.CCE)}
    for case, member in TC.ISOLATION:
        assert len(case.members) == 5 and len({m[0] for m in case.members}) > 1
    assert TC.ISOLATION[1][0].batch == 100
    for c in cases + [TC.SECOND_STEP, TC.TRAJECTORY] + [c for c, _ in TC.ISOLATION]:   # every member is legal
        for m in c.members:
            TopclassSpec(kernel_size=m[0], input_shape=c.shape, classes=c.classes).geometry()
