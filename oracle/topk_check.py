"""CPU ORACLE -- test infrastructure, NOT part of the product.

Checks of the recommend step's output (top-k ids and their scores) against
the float64 oracle (cf_oracle.predict / recommend) on tables where float32
rounding is visible, used by tests/test_gpu_topk.py and
tests/test_gpu_bench_configs.py.

With E = fp32_bound.score_bound (|fp32 score - float64 score| <= E for any
float32 evaluation):

* every returned value is within E of the oracle's score of the returned id;
* the p-th largest elements of two arrays that differ elementwise by at most
  Emax differ by at most Emax, so the item g at position p of a correct
  float32 list and the oracle's item o there satisfy
  |S[g] - S[o]| <= |S[g] - s32[g]| + |s32[g] - S[o]| <= 2 Emax,
  Emax = max_j E[r, j].  A positional mismatch is allowed only inside that.

Tables whose scores are exact in float32 need none of this
(tests/test_gpu_topk_exact.py).
"""
import os

import numpy as np


def check_lists(gpu_idx, scores, oracle_lists, atol, bound=None, excluded=None):
    """Exact order, except that a position may hold another item whose fp64
    score is within the near-tie width of the oracle's item there:
    min(atol, 2 max_j bound[r, j]) -- atol alone without a bound.  No row may
    repeat an id or hold one of its excluded ids (``excluded``: per row, the
    ids the call excluded).  Returns (mismatched positions, compared
    positions)."""
    bad = total = 0
    for r, (g, o) in enumerate(zip(gpu_idx, oracle_lists)):
        g = [int(x) for x in g if x >= 0]
        assert len(g) == len(o), (r, len(g), len(o))
        assert len(set(g)) == len(g), ("repeated id", r)
        if excluded is not None:
            hit = np.intersect1d(np.asarray(g, dtype=np.int64), np.asarray(excluded[r], dtype=np.int64))
            assert hit.size == 0, ("excluded id returned", r, hit[:8].tolist())
        total += len(o)
        if g == o:
            continue
        s = scores[r]
        tie = atol if bound is None else min(atol, 2.0 * float(np.max(bound[r])))
        for a, b in zip(g, o):
            if a != b:
                assert abs(s[a] - s[b]) <= tie, (r, a, b, s[a], s[b], tie)
                bad += 1
    return bad, total


def check_values(gpu_val, gpu_idx, scores, bound, what=""):
    """|val - S[r, idx]| <= bound[r, idx] at every filled position, NaN at
    every padded one (idx -1).  Returns the worst |val - S| / bound."""
    gpu_idx = np.asarray(gpu_idx)
    gpu_val = np.asarray(gpu_val, dtype=np.float64)
    assert gpu_val.shape == gpu_idx.shape
    pad = gpu_idx < 0
    assert np.isnan(gpu_val[pad]).all(), (what, "a padded position holds a value")
    rows = np.nonzero(~pad)[0]
    ids = gpu_idx[~pad]
    err = np.abs(gpu_val[~pad] - scores[rows, ids])     # NaN where a filled value is NaN
    E = bound[rows, ids]
    ok = err <= E
    if not ok.all():
        q = int(np.nonzero(~ok)[0][0])
        raise AssertionError("%s: %d of %d values outside the a-priori fp32 bound; first at row %d id %d: "
                             "gpu %.9g, oracle %.9g, E %.3g"
                             % (what, int((~ok).sum()), ok.size, rows[q], ids[q], gpu_val[~pad][q],
                                scores[rows[q], ids[q]], E[q]))
    nz = E > 0
    worst = float((err[nz] / E[nz]).max()) if nz.any() else 0.0
    log = os.environ.get("CF_BOUND_LOG")
    if log:   # the worst |gpu - oracle| / E per call
        with open(log, "a") as f:
            f.write("%s topk-values %s %.4f\n" % (os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0],
                                                 what, worst))
    return worst
