"""The MFMA-distance clamp of ``gp_score_kernel<.., MD = 1, ..>`` is an inline-asm
``v_max_f64`` on the accumulator of ``v_mfma_f64_16x16x4_f64``.  The compiler does not
count inline asm among the VALU readers of an MFMA result, so ``clamp_r2x4`` (gp.hip)
puts the wait states in front of it itself.  This checks the generated code of every
spill-free MD = 1 instance in libmpo.so: between a ``v_mfma_f64_16x16x4_f64`` and a
``v_max_f64`` that reads one of its result registers lie at least 19 wait states (what
the compiler itself inserts in front of a VALU read it knows about: ``s_nop 15`` +
``s_nop 2`` + the reading instruction's own slot).  CPU only."""
import os
import re

import pytest

from tests import isa_ring as R

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mpi_opt_amd", "libmpo.so")
NEED = 19


def _early_reads(insns):
    """(clamps seen, [(addr, wait states)] of clamps that read an MFMA result too early), in layout order."""
    since = {}
    seen, bad = 0, []
    for addr, mn, ops, _ in insns:
        if mn == "v_max_f64" and re.search(r"s\[\d+:\d+\]\s*$", ops):
            srcs = R.vregs(ops.split(",", 1)[1])
            if srcs & since.keys():
                seen += 1
                w = min(since[r] for r in srcs & since.keys())
                if w < NEED:
                    bad.append((hex(addr), w))
        step = int(ops.strip() or 0) + 1 if mn == "s_nop" else 1
        for r in since:
            since[r] += step
        if mn.startswith("v_mfma_f64_16x16x4"):
            for r in R.vregs(ops.split(",", 1)[0]):
                since[r] = 0
    return seen, bad


def test_counter_sees_an_early_read():
    mfma = [0, "v_mfma_f64_16x16x4_f64", "v[0:7], v[8:9], v[10:11], v[0:7]", None]
    vmax = [40, "v_max_f64", "v[20:21], v[2:3], s[4:5]", None]
    assert _early_reads([mfma, vmax]) == (1, [("0x28", 0)])
    assert _early_reads([mfma, [8, "s_nop", "15", None], [12, "s_nop", "1", None], vmax]) == (1, [("0x28", 18)])
    assert _early_reads([mfma, [8, "s_nop", "15", None], [12, "s_nop", "2", None], vmax]) == (1, [])


@pytest.mark.skipif(not os.path.exists(LIB), reason="libmpo.so not built")
def test_clamp_waits_for_the_mfma_result():
    checked = 0
    for co in R.gfx950_code_objects(LIB):
        for name, insns in R.functions(R.disassemble(co)).items():
            if "gp_score_kernel" not in name or any(i[1].startswith("scratch_") for i in insns):
                continue
            md = int(re.findall(r"Li(\d+)E", name.split("gp_score_kernel")[1])[3])
            seen, bad = _early_reads(insns)
            assert bad == [], (name, bad)
            if md:
                assert seen >= 4, (name, seen)
                checked += 1
    assert checked >= 8          # (8, 5) and (12, 10), FIN 0 / 1, the spill-free occupancy variants
