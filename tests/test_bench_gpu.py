"""GPU: a plain bench.py run times exactly --steps steps, runs none of the --full windows, and --dump-outputs writes what the last timed
step returned (the same tensors --check-sum sums)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_last_timed_step(tmp_path):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "s10k", "--check-sum",
           "--dump-outputs", str(tmp_path / "dump")]
    out = subprocess.run(cmd, check=True, cwd=REPO, timeout=600, capture_output=True, text=True).stdout
    b = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    assert b["steps"] == 3 and b["ms_per_step"] > 0 and b["unit"] == "rays/s" and b["higher_is_better"] is True and b["dtype"] == "f32"
    assert b["sustained"] is None and not {"drop_in_path", "value_varying", "value_deferred_accum", "value_deterministic",
                                           "value_sort_every_build", "cpu_baseline"} & set(b)
    d = {f[:-4]: np.load(str(tmp_path / "dump" / f)) for f in os.listdir(tmp_path / "dump")}
    assert {"out", "accum", "grad_means", "grad_scales", "grad_rotations", "grad_opacities", "grad_shs"} == set(d)
    assert all(v.dtype == np.float32 for v in d.values())
    assert d["out"].shape == (16, 256, 9) and d["grad_shs"].shape == (10_000, 16, 3)       # S10k: below the sampling threshold, whole arrays
    cks = b["checksums"]
    for name, key in (("out", "out"), ("grad_means", "d_means"), ("grad_shs", "d_shs")):
        assert abs(np.abs(d[name].astype(np.float64)).sum() - cks[key]) <= 1e-9 * abs(cks[key]), name
    assert abs(d["accum"].astype(np.float64).sum() - cks["accum"]) <= 1e-9 * abs(cks["accum"])
