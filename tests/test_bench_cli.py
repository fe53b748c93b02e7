"""bench.py's command line: a plain run is the headline EI leg alone (result line,
``--dump-outputs``), every other leg is refused without ``--full``."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench(*argv):
    return subprocess.run([sys.executable, BENCH, *argv], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("argv", [("--workload", "train"), ("--steps", "0"),
                                  ("--full", "--workload", "fit", "--dump-outputs", "unused")])
def test_argument_errors(argv):
    r = _bench(*argv)
    assert r.returncode == 2 and "error" in r.stderr and not r.stdout


@pytest.mark.gpu
def test_plain_run_result_line_and_dump(tmp_path):
    """Two plain runs at a reduced candidate count: one JSON line with the headline
    keys and nothing that belongs to --full, --steps timed steps, and the same
    float64 outputs from both (seeded inputs)."""
    lines, dumps = [], []
    for name in ("a", "b"):
        r = _bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--candidates", "5000",
                   "--dump-outputs", str(tmp_path / name))
        assert r.returncode == 0, r.stderr[-2000:]
        out = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(out) == 1
        lines.append(json.loads(out[0]))
        dumps.append({f[:-4]: np.load(tmp_path / name / f) for f in sorted(os.listdir(tmp_path / name))})
    res = lines[0]
    assert res["steps"] == 3 and res["warmup"] == 1 and res["unit"] == "candidates/s" and res["dtype"] == "f64"
    assert res["higher_is_better"] is True and res["metric"].startswith("EI candidates/sec")
    assert res["ms_per_step"] > 0 and abs(res["value"] - 5000 / (res["ms_per_step"] / 1e3)) <= 1e-6 * res["value"]
    assert not {"roofline", "cpu_baseline", "ask_step_ms", "summary", "train", "densenet"} & set(res)
    a, b = dumps
    assert sorted(a) == ["ei_values", "mu", "sd", "topk_index", "topk_value"]
    for k in a:
        assert a[k].dtype == np.float64 and np.array_equal(a[k], b[k])
    assert a["mu"].shape == a["sd"].shape == a["ei_values"].shape == (5000,)
    # the top-k is skopt's argsort[:5] of the dumped values (lowest index first among ties)
    assert np.array_equal(a["topk_index"], np.argsort(a["ei_values"], kind="stable")[:5])
    assert np.array_equal(a["topk_value"], a["ei_values"][a["topk_index"].astype(int)])
