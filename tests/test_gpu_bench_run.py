"""bench.py end to end on the GPU, on a small rehearsal graph (20,000 users x
2,000 items, 8,192 pairs per step): what a plain run does, what --full adds
and what --dump-outputs writes.

* a plain run prints one line with the headline fields and leaves out every
  pass beside the timed region;
* --dump-outputs writes the tables and the loss of the timed path; the inputs
  are identical from run to run, so in deterministic mode (bitwise
  reproducible steps) two runs write bit-identical files;
* --full adds the per-kernel breakdown, the second batch size and the batch
  statistics to the same line.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "6", "--warmup", "2", "--n-users", "20000", "--n-items", "2000",
         "--batch", "8192", "--secondary-batch", "4096"]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + list(extra),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, universal_newlines=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_is_lean_and_dumps_reproducible_outputs(tmp_path):
    recs = [_bench("--deterministic", "1", "--dump-outputs", str(tmp_path / run)) for run in ("a", "b")]
    for rec in recs:
        for k in HEADLINE:
            assert k in rec, k
        assert rec["steps"] == 6 and rec["warmup"] == 2
        assert rec["unit"] == "triplets/s" and rec["higher_is_better"] is True and rec["dtype"] == "f32"
        assert rec["ms_per_step"] > 0
        assert rec["value"] == pytest.approx(8192 * 6 / (1e-3 * rec["ms_per_step"] * 6))
        # nothing beside the timed region ran
        assert rec["kernels"] == {} and rec["batch_65536"] is None and rec["dedup_step"] is None
        assert rec["roofline_apply_prep"] is None
        assert "cpu_baseline" not in rec and "ndcg10_vs_ref" not in rec and "score_pass" not in rec
    names = sorted(os.listdir(str(tmp_path / "a")))
    assert names == ["acc_item.npy", "acc_user.npy", "item.npy", "loss.npy", "user.npy"]
    total = 0
    for n in names:
        a = np.load(str(tmp_path / "a" / n))
        b = np.load(str(tmp_path / "b" / n))
        total += a.nbytes
        assert a.dtype == (np.float64 if n == "loss.npy" else np.float32), n
        assert np.isfinite(a).all(), n
        assert np.array_equal(a, b), n + ": two runs with the same arguments differ"
    assert total <= 64 << 20
    U = np.load(str(tmp_path / "a" / "user.npy"))
    A = np.load(str(tmp_path / "a" / "acc_user.npy"))
    assert U.shape == (20000, 64) and A.shape == U.shape
    assert (A > 0.1).any(), "the accumulators never moved: no step reached the tables"


def test_full_run_adds_the_other_passes():
    rec = _bench("--full", "--no-cpu-baseline", "--no-ndcg")
    for k in HEADLINE:
        assert k in rec, k
    assert rec["kernels"].get("step", {}).get("launches", 0) > 0
    assert rec["batch_65536"]["batch_pairs_per_gpu"] == 4096 and rec["batch_65536"]["ms_per_step"] > 0
    assert rec["dedup_step"]["unique_rows"] > 0
